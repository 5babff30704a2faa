"""The reference's single-agent benchmark search (include/neptune_hastar.h): AstarPathFinder, a grid A* with a homotopy signature
and a contact-point tether-length check, thousands of searches per launch.

    ha = HomotopicAstar(make_cfg(...), n_scenes).set_statics(scene, uninflated, reps, drone_radius=...)
    results, paths, states = ha.search(scene, start, goal)                  # one wave per search on the GPU
    results2, paths2, states2 = ha.search(scene, goal, goal2, state=states) # chained: the terminal state is the next initial one

`device=False` runs the host form (no GPU, no HIP call); both forms agree on every byte.  States are numpy structured arrays
(state_dtype): n_hsig, hsig_id, hsig_sign, n_cont, cont — eu::ent_state_orig with this build's capacities."""
import ctypes as C

import numpy as np

from . import abi
from ._lib import BackendError, check, lib


def make_cfg(resolution, x_min, x_max, y_min, y_max, z_min, z_max, cable_length, bias=1.1, max_pops=1 << 20, max_nodes=0,
             hsig_cap=32, cont_cap=128, path_cap=256):
    """nep_hastar_cfg; the reference's set-up is resolution = a_star_fraction_voxel_size * 2, bias 1.1, max_nodes 0 (GLX * GLY * GLZ)"""
    return abi.nep_hastar_cfg(float(resolution), float(x_min), float(x_max), float(y_min), float(y_max), float(z_min), float(z_max),
                              float(cable_length), float(bias), int(max_pops), int(max_nodes), int(hsig_cap), int(cont_cap), int(path_cap))


def state_dtype(hsig_cap, cont_cap):
    return np.dtype([("n_hsig", np.int32), ("hsig_id", np.int16, (hsig_cap,)), ("hsig_sign", np.int8, (hsig_cap,)),
                     ("n_cont", np.int32), ("cont", np.float64, (cont_cap, 2))])


def polys_csr(polys):
    """a list of [nv][2] polygons -> (off [n + 1] int32, xy [sum nv][2] float64)"""
    off = np.zeros(len(polys) + 1, dtype=np.int32)
    for k, q in enumerate(polys):
        off[k + 1] = off[k] + len(np.asarray(q).reshape(-1, 2))
    xy = np.zeros((max(int(off[-1]), 1), 2), dtype=np.float64)
    for k, q in enumerate(polys):
        xy[off[k]:off[k + 1]] = np.asarray(q, dtype=np.float64).reshape(-1, 2)
    return off, xy


def inflate(poly, drone_radius):
    """nep_hastar_inflate: the 2 * drone_radius inflation of neptune_ros.cpp:313-343"""
    q = np.ascontiguousarray(poly, dtype=np.float64).reshape(-1, 2)
    out = np.zeros((4 * len(q), 2), dtype=np.float64)
    n = check(lib().nep_hastar_inflate(len(q), abi.dptr(q), float(drone_radius), abi.dptr(out), len(out)))
    return out[:n].copy()


class HomotopicAstar:
    def __init__(self, cfg, scenes=1, base=(0.0, 0.0)):
        self.L = lib()
        self.cfg = cfg
        self.n_scenes = int(scenes)
        self.base = base      # where the tether is anchored: a search without a state starts from contPts = [base]
        self.h = self.L.nep_hastar_create(C.byref(cfg), self.n_scenes)
        if not self.h:
            raise BackendError("nep_hastar_create: " + self.L.nep_last_error().decode())
        self.dtype = state_dtype(cfg.hsig_cap, cfg.cont_cap)

    def close(self):
        if self.h:
            self.L.nep_hastar_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- statics ----
    def set_statics(self, scene=-1, uninflated=(), reps=None, inflated=None, drone_radius=None):
        """uninflated: the obstacles' polygons (updateContPts_orig tests them); inflated: what occupancy tests — given, or made
        from `uninflated` with drone_radius; reps [n][2][2] (None: none).  scene -1: every scene."""
        if inflated is None:
            if drone_radius is None:
                raise ValueError("inflated polygons or a drone_radius to make them")
            inflated = [inflate(q, drone_radius) for q in uninflated]
        off, xy = polys_csr(inflated)
        check(self.L.nep_hastar_set_inflated(self.h, int(scene), len(inflated), abi.iptr(off), abi.dptr(xy)))
        off, xy = polys_csr(uninflated)
        check(self.L.nep_hastar_set_uninflated(self.h, int(scene), len(uninflated), abi.iptr(off), abi.dptr(xy)))
        r = np.zeros((0, 2, 2)) if reps is None else np.ascontiguousarray(reps, dtype=np.float64).reshape(-1, 2, 2)
        rr = r if len(r) else np.zeros((1, 2, 2))
        check(self.L.nep_hastar_set_reps(self.h, int(scene), len(r), abi.dptr(rr)))
        return self

    def search_bytes(self):
        return int(self.L.nep_hastar_search_bytes(self.h))

    # ---- states ----
    def initial_state(self, n, base, hsig=()):
        """n states with contPts = [base] (neptune_ros.cpp:353) and the signature `hsig`, a list of (rep id from 1, sign)"""
        st = np.zeros(n, dtype=self.dtype)
        st["n_cont"] = 1
        st["cont"][:, 0, :] = np.asarray(base, dtype=np.float64).reshape(-1, 2)
        st["n_hsig"] = len(hsig)
        for e, (i, s) in enumerate(hsig):
            st["hsig_id"][:, e] = i
            st["hsig_sign"][:, e] = s
        return st

    def _soa(self, st):
        """a structured state array -> the five contiguous arrays of the struct-of-arrays form"""
        # (copies: a field of a one-element structured array counts as contiguous while it keeps the record's stride)
        return [np.array(st[k], order="C", copy=True) for k in ("n_hsig", "hsig_id", "hsig_sign", "n_cont", "cont")]

    def _struct(self, ptrs):
        return abi.nep_hastar_state(self.cfg.hsig_cap, self.cfg.cont_cap, *ptrs)

    def _inputs(self, scene, start, goal, state):
        start = np.ascontiguousarray(start, dtype=np.float64).reshape(-1, 2)
        n = len(start)
        goal = np.ascontiguousarray(np.broadcast_to(np.asarray(goal, dtype=np.float64).reshape(-1, 2), (n, 2)))
        scene = np.ascontiguousarray(np.broadcast_to(np.asarray(scene, dtype=np.int32).reshape(-1), (n,)))
        if state is None:
            state = self.initial_state(n, self.base)
        return n, scene, start, goal, state

    # ---- searches ----
    def search(self, scene, start, goal, state=None, device=True):
        """scene [n] (or one), start, goal [n][2], state [n] of state_dtype -> (results [n] HASTAR_RESULT_DTYPE, paths
        [n][path_cap][2], terminal states [n])"""
        n, scene, start, goal, state = self._inputs(scene, start, goal, state)
        if device:
            d = self.search_device(scene, start, goal, self.to_device_state(state))
            self.synchronize()
            return self.from_device(d)
        assert state.dtype == self.dtype and state.shape == (n,)
        sin = self._soa(state)
        sout = [np.zeros_like(a) for a in sin]
        res = np.zeros(n, dtype=abi.HASTAR_RESULT_DTYPE)
        path = np.zeros((n, self.cfg.path_cap, 2), dtype=np.float64)
        check(self.L.nep_hastar_search_host(self.h, n, scene.ctypes.data, start.ctypes.data, goal.ctypes.data,
                                            C.byref(self._struct([a.ctypes.data for a in sin])), res.ctypes.data, path.ctypes.data,
                                            C.byref(self._struct([a.ctypes.data for a in sout]))))
        return res, path, self._join(sout)

    def _join(self, soa):
        st = np.zeros(len(soa[0]), dtype=self.dtype)
        for k, a in zip(("n_hsig", "hsig_id", "hsig_sign", "n_cont", "cont"), soa):
            st[k] = a
        return st

    def to_device_state(self, state):
        """a structured state array -> the struct-of-arrays form on the device (a list of five tensors)"""
        import torch
        assert state.dtype == self.dtype
        return [torch.from_numpy(a).cuda() for a in self._soa(state)]

    def search_device(self, scene, start, goal, d_state, d_state_out=None, out=None, stream=None):
        """Everything stays on the device.  d_state: five tensors (to_device_state, or the "state" of an earlier call's return).
        Returns a dict of tensors: result (bytes), path, state.  `out`: an earlier return to write into again (same n): no
        allocation, so that the call can be captured."""
        import torch
        n = d_state[0].shape[0]
        dev = lambda a, dt: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, dtype=dt, order="C", copy=True)).cuda()      # noqa: E731
        scene, start, goal = dev(scene, np.int32), dev(start, np.float64), dev(goal, np.float64)
        if out is None:
            out = dict(result=torch.zeros(n * abi.HASTAR_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda"),
                       path=torch.zeros((n, self.cfg.path_cap, 2), dtype=torch.float64, device="cuda"),
                       state=d_state_out if d_state_out is not None else [torch.zeros_like(t) for t in d_state])
        out["inputs"] = (scene, start, goal, d_state)      # kept alive for as long as the launch may run
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        check(self.L.nep_hastar_search(self.h, n, scene.data_ptr(), start.data_ptr(), goal.data_ptr(),
                                       C.byref(self._struct([t.data_ptr() for t in d_state])), out["result"].data_ptr(), out["path"].data_ptr(),
                                       C.byref(self._struct([t.data_ptr() for t in out["state"]])), s))
        return out

    def from_device(self, d):
        res = d["result"].cpu().numpy().view(abi.HASTAR_RESULT_DTYPE).copy()
        return res, d["path"].cpu().numpy(), self._join([t.cpu().numpy() for t in d["state"]])

    def synchronize(self):
        import torch
        torch.cuda.synchronize()

    def check(self, stream=None):
        """NEP_E_CAP (BackendError) when a search since the last check hit a capacity"""
        s = 0
        if stream is not None:
            s = stream
        else:
            try:
                import torch
                if torch.cuda.is_available():
                    s = torch.cuda.current_stream().cuda_stream
            except ImportError:
                pass
        return check(self.L.nep_hastar_check(self.h, s))

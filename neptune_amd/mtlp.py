"""The comparator of the reference's main benchmark (include/neptune_mtlp.h): mtlp::solveMultiTetherLinearPath, the sequential
planner of Hert and Lumelsky for several tethered robots in R3, thousands of runs per launch.

    m = Mtlp(make_cfg(0.2, -10, 10, -10, 10, 0, 3, radius=0.2, n_robots=5, max_pops=4000, max_nodes=20000))
    out = m.solve(bases, start_goal)                # bases [R][N][3], start_goal [R][N][2][3]; one wave per (run, robot)
    out["graph"], out["run_status"], out["result"], out["path"]

`device=False` runs the host form (no GPU, no HIP call); both forms agree on every byte.  The geometric tests are exact
(a filtered double evaluation, then fixed-width integers): inputs are multiples of 2^-60 of magnitude <= 1e5."""
import ctypes as C

import numpy as np

from . import abi
from ._lib import BackendError, check, lib


def make_cfg(resolution, x_min, x_max, y_min, y_max, z_min, z_max, radius, n_robots, max_pops, max_nodes=0, bias=1.1, path_cap=256):
    """nep_mtlp_cfg; the reference's set-up is resolution = a_star_fraction_voxel_size, radius = drone_radius, bias 1.1, max_nodes 0
    (GLX * GLY * GLZ).  max_pops has no default: the reference has no such budget, a device search needs one."""
    return abi.nep_mtlp_cfg(float(resolution), float(x_min), float(x_max), float(y_min), float(y_max), float(z_min), float(z_max),
                            float(radius), float(bias), int(n_robots), int(max_nodes), int(max_pops), int(path_cap))


def circle_bases(n):
    """nep_mtlp_circle_bases: the bases of the reference's circle_init_bases, [n][3]"""
    out = np.zeros((n, 3), dtype=np.float64)
    check(lib().nep_mtlp_circle_bases(int(n), abi.dptr(out)))
    return out


def predicates(which, records, device=False):
    """Debug: records [n][16] -> (verdict [n], exact [n]); which 0 segment/triangle, 1 segment/segment in 2-D, 2 ball/segment"""
    rec = np.ascontiguousarray(records, dtype=np.float64).reshape(-1, 16)
    n = len(rec)
    if not device:
        v = np.zeros(n, dtype=np.int32); e = np.zeros(n, dtype=np.int32)
        check(lib().nep_mtlp_predicates_host(int(which), n, rec.ctypes.data, v.ctypes.data, e.ctypes.data))
        return v, e
    import torch
    d = torch.from_numpy(rec).cuda()
    v = torch.zeros(n, dtype=torch.int32, device="cuda"); e = torch.zeros(n, dtype=torch.int32, device="cuda")
    check(lib().nep_mtlp_predicates_device(int(which), n, d.data_ptr(), v.data_ptr(), e.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return v.cpu().numpy(), e.cpu().numpy()


class Mtlp:
    def __init__(self, cfg):
        self.L = lib()
        self.cfg = cfg
        self.n = int(cfg.n_robots)
        self.h = self.L.nep_mtlp_create(C.byref(cfg))
        if not self.h:
            raise BackendError("nep_mtlp_create: " + self.L.nep_last_error().decode())

    def close(self):
        if self.h:
            self.L.nep_mtlp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def search_bytes(self):
        return int(self.L.nep_mtlp_search_bytes(self.h))

    def _inputs(self, bases, start_goal):
        bases = np.ascontiguousarray(bases, dtype=np.float64).reshape(-1, self.n, 3)
        sg = np.ascontiguousarray(start_goal, dtype=np.float64).reshape(-1, self.n, 2, 3)
        assert len(bases) == len(sg)
        return len(bases), bases, sg

    def solve(self, bases, start_goal, device=True):
        """bases [R][N][3], start_goal [R][N][2][3] -> dict: graph [R][N][N] int32, run_status [R] int32, result [R][N]
        MTLP_RESULT_DTYPE, path [R][N][path_cap][3]"""
        r, bases, sg = self._inputs(bases, start_goal)
        if device:
            d = self.solve_device(bases, sg)
            self.synchronize()
            return self.from_device(d)
        out = dict(graph=np.zeros((r, self.n, self.n), dtype=np.int32), run_status=np.zeros(r, dtype=np.int32),
                   result=np.zeros((r, self.n), dtype=abi.MTLP_RESULT_DTYPE), path=np.zeros((r, self.n, self.cfg.path_cap, 3), dtype=np.float64))
        check(self.L.nep_mtlp_solve_host(self.h, r, bases.ctypes.data, sg.ctypes.data, out["graph"].ctypes.data, out["run_status"].ctypes.data,
                                         out["result"].ctypes.data, out["path"].ctypes.data))
        return out

    def alloc_device(self, r):
        """the four output tensors of r runs (result as bytes)"""
        import torch
        return dict(graph=torch.zeros((r, self.n, self.n), dtype=torch.int32, device="cuda"), run_status=torch.zeros(r, dtype=torch.int32, device="cuda"),
                    result=torch.zeros(r * self.n * abi.MTLP_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda"),
                    path=torch.zeros((r, self.n, self.cfg.path_cap, 3), dtype=torch.float64, device="cuda"))

    def solve_device(self, bases, start_goal, out=None, stream=None):
        """Everything stays on the device.  bases, start_goal: tensors (or arrays, uploaded).  `out`: an earlier return (or
        alloc_device) to write into: no allocation, so that the call can be captured.  Returns the dict of tensors."""
        import torch
        dev = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, dtype=np.float64, order="C", copy=True)).cuda()      # noqa: E731
        bases, sg = dev(bases), dev(start_goal)
        r = bases.numel() // (3 * self.n)
        assert sg.numel() == 6 * self.n * r and bases.is_contiguous() and sg.is_contiguous()
        if out is None:
            out = self.alloc_device(r)
        out["inputs"] = (bases, sg)      # kept alive for as long as the launch may run
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        check(self.L.nep_mtlp_solve(self.h, r, bases.data_ptr(), sg.data_ptr(), out["graph"].data_ptr(), out["run_status"].data_ptr(),
                                    out["result"].data_ptr(), out["path"].data_ptr(), s))
        return out

    def from_device(self, d):
        r = d["run_status"].shape[0]
        return dict(graph=d["graph"].cpu().numpy(), run_status=d["run_status"].cpu().numpy(),
                    result=d["result"].cpu().numpy().view(abi.MTLP_RESULT_DTYPE).reshape(r, self.n).copy(), path=d["path"].cpu().numpy())

    def synchronize(self):
        import torch
        torch.cuda.synchronize()

    def check(self, stream=None):
        """NEP_E_CAP (BackendError) when a search since the last check set PATH or STATE"""
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
        return check(self.L.nep_mtlp_check(self.h, s))

"""Development aid: thread 0's shader cycles per phase of the polish pass, both forms, mean over the listed slots of eight 64-agent
scenes on front-end guesses.  Needs a library built with  make PROFILE=1 EXTRA=-DNEP_POLISH_PROF  (NEP_BACKEND_LIB points at it).
python scripts/polish_phases.py [scenes=8] [cull=4.0]"""
import os, sys
os.environ["NEP_QP_PROFILE"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np
from neptune_amd import abi, scene, dist as ndist, _lib
from neptune_amd.backend import BatchBackend

PHASES = ("entry loads", "line staging", "table staging", "active-set scan", "rounds", "theta + verification", "stores")


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    cull = float(sys.argv[2]) if len(sys.argv) > 2 else 4.0
    scs = [scene.make_scene(64, 20, seed=200 + s) for s in range(S)]
    com, gue = ndist.stack_scenes(scs)
    L = _lib.lib()
    g = None
    for impl in (0, 1):
        assert L.nep_debug_set_global_option(b"polish_impl", impl) == 0
        be = BatchBackend(scs[0]["par"], scs[0]["statics"], n_scenes=S)
        for s in range(1, S):
            be.set_scene_statics(s, scs[s]["statics"])
        d_com = be.to_device(com)
        if g is None:
            d_g = be.to_device(gue)
            be.frontend(scene.frontend_cfg(scs[0]["par"], beam_width=32), d_com, be.to_device(np.stack([scene.frontend_starts(s) for s in scs])), d_g, None)
            g = d_g.cpu().numpy().view(abi.GUESS_DTYPE).copy()
        be.set_line_cull(cull)
        d_g = be.to_device(g)
        for _ in range(3):
            be.replan(d_com, d_g)
        fl = be.polish_flags()
        listed = np.flatnonzero(fl)
        c = np.array([be.debug_phase_cycles(be.slots + int(s))[:8] for s in listed], dtype=np.int64)
        c = c[c[:, 7] == 1]
        print("polish_impl %d, cull %.1f: %d listed, %d certified; mean shader cycles per listed slot (%d rows read):" % (impl, cull, len(listed), int(((fl & 0x100) != 0).sum()), len(c)))
        for k, name in enumerate(PHASES):
            print("  %-22s %8.0f   (max %d)" % (name, c[:, k].mean(), c[:, k].max()))
        print("  %-22s %8.0f" % ("sum", c[:, :7].sum(axis=1).mean()), flush=True)
        be.close()
    L.nep_debug_set_global_option(b"polish_impl", 1)


if __name__ == "__main__":
    main()

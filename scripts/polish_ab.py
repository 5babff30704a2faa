"""Development aid: the polish pass's forms on the bench's scenes, same process, alternating (A/B of the global debug options
"polish_impl" and "parked_bound", include/neptune_backend_debug.h): HIP-event time of the QP phase (main launch + redo + polish) and
of the whole sequence, the polish counts and a digest of the coefficients per variant.
python scripts/polish_ab.py [scenes=128] [rounds=3] [agents=64] [statics=20] [cull=<radius>]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np
from neptune_amd import scene, dist as ndist, _lib
from neptune_amd.backend import BatchBackend

VARIANTS = (("polish_impl=0", 0, 1), ("polish_impl=1 parked_bound=0", 1, 0), ("polish_impl=1 parked_bound=1", 1, 1))


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    N = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    M = int(sys.argv[4]) if len(sys.argv) > 4 else 20
    cull = float(sys.argv[5]) if len(sys.argv) > 5 else None
    scs = scene.make_scenes(N, M, range(S), workers=min(S, 16))
    com, gue = ndist.stack_scenes(scs)
    L = _lib.lib()
    for r in range(rounds):
        for name, impl, bound in VARIANTS:
            assert L.nep_debug_set_global_option(b"polish_impl", impl) == 0 and L.nep_debug_set_global_option(b"parked_bound", bound) == 0
            be = BatchBackend(scs[0]["par"], scs[0]["statics"], n_scenes=S)
            for s in range(1, S):
                be.set_scene_statics(s, scs[s]["statics"])
            if cull is not None:
                be.set_line_cull(cull)
            d_com, d_gue = be.to_device(com), be.to_device(gue)
            for _ in range(5):
                be.replan(d_com, d_gue)
            be.enable_timing(True); be.reset_timing()
            for _ in range(40):
                be.replan(d_com, d_gue)
            t = [be.kernel_time_ms(i)[0] for i in range(4)]
            be.enable_timing(False)
            sol = be.solutions()
            print("round %d %-30s qp(+redo+polish) %.4f  sequence %.4f ms | polish %r, redo %d, digest %016x"
                  % (r, name, t[2], t[3], be.polish_count(), be.redo_count(),
                     int(np.frombuffer(np.ascontiguousarray(sol["coeff"]).tobytes(), dtype=np.uint64).sum() & 0xFFFFFFFFFFFFFFFF)), flush=True)
            be.close()
    L.nep_debug_set_global_option(b"polish_impl", 1); L.nep_debug_set_global_option(b"parked_bound", 1)


if __name__ == "__main__":
    main()

"""The parameter table of the sweep (test_oracle_params.py, test_gpu_param_sweep.py, golden/make_golden_params.py): named
scene.Params overrides away from the one point every other test uses (scene.Params' defaults = the reference's mtlp benchmark
yaml).  The values are those the reference's other parameter files fly (typed in here; no file of the reference is read) and a
few corners of our own.  One place: everything that sweeps takes its sets from here."""
from neptune_amd import scene

SETS = {
    "default": {},
    # the reference's hardware-experiment values: short horizon, fine sampling, slow, small drone, low ceiling, short tether
    "exp": dict(T_span=0.3, dc=0.02, v_max=0.7, a_max=2.0, j_max=3.5, drone_radius=0.35, z_min=-0.2, z_max=1.8, tether_length=7.0),
    # its single-agent / multi-obstacle benchmarks: smaller drone, a z box that reaches below the floor
    "single": dict(drone_radius=0.5, z_min=-1.0, z_max=2.5),
    # a guess travels tens of metres: most separating lines lie beyond the 4 m cull radius of the line presolve
    "fast_long": dict(T_span=1.0, v_max=5.0, a_max=6.0, weight=10.0),
    "heavy": dict(weight=1e5),
    # handles created with fewer intervals than NEP_MAX_POL (other max_states, hull grid, bucket strides)
    "pol5": dict(num_pol=5),
    "pol6": dict(num_pol=6),
}

# guess lengths flown per set (K <= num_pol)
GUESS_K = {"pol5": (5,), "pol6": (4, 6)}

SWEPT = ("exp", "single", "fast_long", "heavy", "pol5", "pol6")


def params(name, num_agents, n_static):
    """scene.scaled_params with the set's overrides"""
    kw = dict(SETS[name])
    tether = kw.pop("tether_length", None)
    p = scene.scaled_params(num_agents, n_static, **kw)
    if tether is not None:
        p.tether_length = tether          # (scaled_params scales the default tether with the world)
    return p


def guess_lengths(name):
    return GUESS_K.get(name, (SETS[name].get("num_pol", 8),))


def make_scene(name, num_agents, n_static, seed, K=None, **kw):
    """scene.make_scene at a set of the table (K: the set's first guess length unless given)"""
    p = params(name, num_agents, n_static)
    return scene.make_scene(num_agents, n_static, seed=seed, K=guess_lengths(name)[0] if K is None else K, par=p, **kw)

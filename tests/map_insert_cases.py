"""The inputs the map-insertion tests share: test_map_insert_cpu.py shows they reach the branches they are named for,
test_gpu_map_insert.py runs the device entry points on them.  A case is (map with slot kf2, kf, map2kf mix): the KF <-> KF insert of
`kf` and then a map <-> KF insert made with synthetic_map2kf from the map the first one leaves.  T = the look-back tile."""
import functools

import numpy as np

from plslam_amd import local_map as LM
from plslam_amd import map_insert as MI

T = MI.LOOKBACK_TILE
N_PT, N_LS = 96, 32                                               # the keyframe of the base cases


@functools.lru_cache(maxsize=None)
def base_map():
    return LM.synthetic_map()                                     # 40 keyframes, 600 points, 150 lines


def _base(points, lines, m2k=None, seed=3, n_pt=N_PT, n_ls=N_LS, m=None):
    m, kf = MI.synthetic_keyframe(base_map() if m is None else m, n_pt, n_ls, seed, points, lines)
    return m, kf, m2k or dict(points=dict(n_events=6, n_invalid=1), lines=dict(n_events=3))


def tile_events(d):
    """T + d events of each kind: existing points, new lines"""
    return _base(dict(n_exist=T + d), dict(n_new=T + d), n_pt=2 * T + 16, n_ls=T + 8, seed=40 + d,
                 m2k=dict(points=dict(n_events=T + d), lines=dict(n_events=3)))


def tile_landmarks(d):
    """T + d landmarks of each kind after the insert (3 of them new): the obs_ptr scan ends at a tile's edge"""
    m = LM.synthetic_map(n_kf=12, n_pt=T + d - 3, n_ls=T + d - 3, seed=60 + d)
    return _base(dict(n_new=3, n_exist=5), dict(n_new=3, n_exist=5), m=m, seed=50 + d)


def big():
    """200 000 point landmarks, 2 000 point events: the event scan crosses 9 tiles, the obs_ptr scan 784"""
    m = LM.synthetic_map(n_kf=60, n_pt=200_000, n_ls=3000, seed=77, max_obs=4)
    return _base(dict(n_new=600, n_exist=1300, n_same_lm=50), dict(n_new=100, n_exist=200), m=m, n_pt=2100, n_ls=400, seed=9,
                 m2k=dict(points=dict(n_events=90, n_same_i2=4), lines=dict(n_events=50)))


def short_arrays():
    """the last three matched features of kf1 lie beyond P1 / obs1 as given: skipped"""
    m, kf, m2k = _base(dict(n_new=20), dict(n_new=8))
    for kind in ("points", "lines"):
        kf[kind] = dict(kf[kind], P1=kf[kind]["P1"][:-3], obs1=kf[kind]["obs1"][:-3])
    return m, kf, m2k


_MIXED_PT = dict(n_new=18, n_exist=18, n_invalid=5, n_out_of_range=4, n_null1=4, n_null2=4, n_i2_out_of_range=3, genuine=0.3)
_MIXED_LS = dict(n_new=5, n_exist=5, n_invalid=3, n_out_of_range=3, n_null1=3, n_null2=3, n_i2_out_of_range=3, genuine=0.2)
_M2K_MIXED = dict(points=dict(n_events=8, n_same_i2=3, n_null2=3, n_i2_out_of_range=3, n_invalid=3),
                  lines=dict(n_events=3, n_same_i2=3, n_null2=3, n_i2_out_of_range=3, n_invalid=3))

CASES = {
    "no_events": lambda: _base({}, {}, m2k=dict(points={}, lines={})),
    "null_kind": lambda: _base(dict(n_new=10, n_exist=10), None, m2k=dict(points=None, lines=None)),
    "only_new": lambda: _base(dict(n_new=40), dict(n_new=12)),
    "only_existing": lambda: _base(dict(n_exist=40), dict(n_exist=12)),
    "mixed": lambda: _base(_MIXED_PT, _MIXED_LS, m2k=_M2K_MIXED),
    "same_landmark": lambda: _base(dict(n_same_lm=6, n_exist=10, n_new=4), dict(n_same_lm=4, n_exist=4)),
    "same_i2": lambda: _base(dict(n_same_i2=6, n_exist=10, n_new=10), dict(n_same_i2=4, n_new=6, n_exist=3),
                             m2k=dict(points=dict(n_events=8, n_same_i2=4), lines=dict(n_events=3, n_same_i2=3))),
    "empty_lists": lambda: _base(dict(n_empty=5, n_exist=5), dict(n_empty=3, n_exist=3)),
    "short_arrays": short_arrays,
    **{f"tile_events_{d:+d}": (lambda d=d: tile_events(d)) for d in (-1, 0, 1)},
    **{f"tile_landmarks_{d:+d}": (lambda d=d: tile_landmarks(d)) for d in (-1, 0, 1)},
}

# the branches (tests/map_insert_ref.py: BRANCHES) each case exists for: taken at least 3 times, in the pass named
REACHES = {
    "no_events": dict(kf2kf=("no_match",), map2kf=("no_match",)),
    "only_new": dict(kf2kf=("kf2kf.new",)),
    "only_existing": dict(kf2kf=("kf2kf.existing", "row.other_kf", "row.same_kf"), map2kf=("map2kf.event",)),
    "mixed": dict(kf2kf=("kf2kf.new", "kf2kf.existing", "kf2kf.lm_null", "kf2kf.lm_range", "skip.kf1_null", "skip.kf2_null",
                         "skip.i2_range", "no_match"),
                  map2kf=("map2kf.event", "map2kf.lm_null_all_the_same", "skip.kf2_null", "skip.i2_range", "same_i2")),
    "same_landmark": dict(kf2kf=("same_lm",)),
    "same_i2": dict(kf2kf=("same_i2",), map2kf=("same_i2",)),
    "empty_lists": dict(kf2kf=("empty_list",)),
    "short_arrays": dict(kf2kf=("skip.i1_range",)),
}


@functools.lru_cache(maxsize=None)
def run_ref(name):
    """-> (m, kf, after the KF <-> KF insert (map, out), kf of the map <-> KF insert, after it (map, out), hits of the two passes);
    computed once per case and shared: nobody writes to it"""
    import collections

    import map_insert_ref as R
    m, kf, m2k = (big if name == "big" else CASES[name])()
    h1, h2 = collections.Counter(), collections.Counter()
    a = R.insert_kf2kf(m, kf, h1)
    kf_b = MI.synthetic_map2kf(a[0], kf, seed=11, points=m2k["points"], lines=m2k["lines"])
    b = R.insert_map2kf(a[0], kf_b, h2)
    return m, kf, a, kf_b, b, (h1, h2)

"""The inputs the loop-closure fusion tests share: test_lc_fuse_cpu.py shows they reach the branches they are named for,
test_gpu_lc_fuse.py runs the device call on them.  A case is (map, lc): the arguments of one plslam_lc_fuse_run.  T = the
look-back tile, L = the level limit."""
import functools

import numpy as np

from plslam_amd import lc_fuse as LF
from plslam_amd import local_map as LM

T = LF.LOOKBACK_TILE
L = LF.MAX_LEVEL
ENTRIES = ((3, 30, 1), (5, 33, 1), (8, 36, 1))                    # kf_prev, kf_curr, flag
NULL = LM.FEAT_NULL


@functools.lru_cache(maxsize=None)
def base_map():
    return LM.synthetic_map()                                     # 40 keyframes, 600 points, 150 lines


def _gen(points, lines, entries=ENTRIES[:1], seed=3, m=None):
    m = base_map() if m is None else m
    return m, LF.synthetic_loop_closure(m, entries, points, lines, seed)


class _Pick:
    """valid landmarks with observations, each handed out once, and non-NULL features of a keyframe, for the explicit cases"""

    def __init__(self, m, kind, seed):
        self.A, self.rng = m[kind], np.random.Generator(np.random.PCG64(seed))
        lens = np.diff(self.A["obs_ptr"])
        self.ok = self.rng.permutation(np.flatnonzero((self.A["valid"] == 1) & (lens > 0))).tolist()

    def lm(self):
        return self.ok.pop()

    def feat(self, kf):
        f = self.A["feat_idx"][self.A["feat_ptr"][kf]:self.A["feat_ptr"][kf + 1]]
        return int(self.rng.choice(np.flatnonzero(f != NULL)))

    def seen_from(self, kf):
        """a landmark not handed out yet that keyframe kf observes"""
        for x in self.ok:
            if kf in self.A["obs_kf"][self.A["obs_ptr"][x]:self.A["obs_ptr"][x + 1]]:
                self.ok.remove(x)
                return x
        raise AssertionError("no landmark seen from the keyframe")


def _explicit(build, entries, seed, sets=(4, 3)):
    """build(pick, s) -> per entry the tuples of set s; `sets` sets of points and of lines, concatenated per entry"""
    m, per = base_map(), {}
    for kind, n_sets in zip(("points", "lines"), sets):
        pick = _Pick(m, kind, seed)
        out = [[] for _ in entries]
        for s in range(n_sets):
            for i, tuples in enumerate(build(pick, s)):
                out[i] += tuples
        per[kind] = out
    return m, LF.pack_loop_closure(m, entries, per["points"], per["lines"], seed)


def same_feature():
    """two events of one entry write one feature of kf_prev (two A) and one of kf_curr (a B and a D): the later index stays"""
    (kp, kc, _), = ENTRIES[:1]

    def build(p, s):
        f0, f1 = p.feat(kp), p.feat(kc)
        return [[(-1, f0, p.lm(), p.feat(kc)), (-1, f0, p.lm(), p.feat(kc)), (p.lm(), p.feat(kp), -1, f1), (p.lm(), p.feat(kp), p.lm(), f1)]]
    return _explicit(build, ENTRIES[:1], 5)


def dead_then_named():
    """a D, then in a later entry an A, a B and two D that name the dead landmark"""
    def build(p, s):
        (kp, kc, _), (kp2, kc2, _) = ENTRIES[:2]
        a, b = p.lm(), p.lm()
        return [[(a, p.feat(kp), b, p.feat(kc))],
                [(-1, p.feat(kp2), b, p.feat(kc2)), (b, p.feat(kp2), -1, p.feat(kc2)), (p.lm(), p.feat(kp2), b, p.feat(kc2)),
                 (b, p.feat(kp2), p.lm(), p.feat(kc2))]]
    return _explicit(build, ENTRIES[:2], 6)


def nested():
    """b into a, then a into c, with appends on each in between: the order of c's list is not the order of the events"""
    def build(p, s):
        (kp, kc, _), (kp2, kc2, _) = ENTRIES[:2]
        a, b, c = p.lm(), p.lm(), p.lm()
        return [[(-1, p.feat(kp), b, p.feat(kc)), (-1, p.feat(kp), c, p.feat(kc)), (a, p.feat(kp), b, p.feat(kc)), (a, p.feat(kp), -1, p.feat(kc))],
                [(c, p.feat(kp2), -1, p.feat(kc2)), (c, p.feat(kp2), a, p.feat(kc2)), (-1, p.feat(kp2), c, p.feat(kc2))]]
    return _explicit(build, ENTRIES[:2], 7)


def grown_then_fused():
    """A and B events on b before it is fused: the fusion copies what they appended"""
    def build(p, s):
        (kp, kc, _), = ENTRIES[:1]
        a, b = p.lm(), p.lm()
        return [[(-1, p.feat(kp), b, p.feat(kc)), (b, p.feat(kp), -1, p.feat(kc)), (a, p.feat(kp), b, p.feat(kc))]]
    return _explicit(build, ENTRIES[:1], 8)


def diagonal():
    """A on a landmark kf_curr observes already, B on one kf_prev does: 2 on the diagonal of the graph"""
    def build(p, s):
        (kp, kc, _), = ENTRIES[:1]
        return [[(-1, p.feat(kp), p.seen_from(kc), p.feat(kc)), (p.seen_from(kp), p.feat(kp), -1, p.feat(kc))]]
    return _explicit(build, ENTRIES[:1], 9)


def chain(length):
    """`length` events on one landmark per kind, alternating A and B over two entries: the last one has level `length`"""
    def build(p, s):
        (kp, kc, _), (kp2, kc2, _) = ENTRIES[:2]
        x, half = p.lm(), length // 2
        return [[((-1, p.feat(kp), x, p.feat(kc)), (x, p.feat(kp), -1, p.feat(kc)))[i % 2] for i in range(half)],
                [((-1, p.feat(kp2), x, p.feat(kc2)), (x, p.feat(kp2), -1, p.feat(kc2)))[i % 2] for i in range(length - half)]]
    return _explicit(build, ENTRIES[:2], 10, sets=(2, 1))


def mixed():
    """every skip reason: a NULL slot (the second entry's kf_prev), indices beyond the map and the keyframes, a == b, an empty b,
    observations of keyframes beyond the map (every 7th entry of obs_kf); NULL features on either side, NULL landmarks"""
    m = LM.synthetic_map(null_kf=(5,), seed=2)
    m = dict(m, points=dict(m["points"], obs_kf=m["points"]["obs_kf"].copy()), lines=dict(m["lines"], obs_kf=m["lines"]["obs_kf"].copy()))
    m["points"]["obs_kf"][::7] = m["n_map_kf"] + 2
    m["lines"]["obs_kf"][::7] = -3
    pt = dict(n_a=12, n_b=12, n_c=8, n_d=12, n_null_feat=3, n_invalid=3, n_lm_range=6, n_ldx_range=8, n_self=3, n_empty=3)
    ls = dict(n_a=3, n_b=3, n_c=3, n_d=3, n_null_feat=3, n_invalid=3, n_lm_range=3, n_ldx_range=4, n_self=3)
    return _gen([pt, dict(n_a=3, n_c=3, n_d=3), dict(pt, n_shared=4)], [ls, dict(n_a=3, n_c=3), dict(n_a=3, n_b=3, n_d=3)],
                entries=ENTRIES, seed=12, m=m)


def tile_events(d):
    """T + d tuples of each kind: A events for the points, C events for the lines"""
    return _gen(dict(n_a=T + d), dict(n_c=T + d), seed=40 + d)


def tile_landmarks(d):
    """T + d landmarks of each kind after the fusion (3 of them new): the obs_ptr scan ends at a tile's edge"""
    m = LM.synthetic_map(n_kf=40, n_pt=T + d - 3, n_ls=T + d - 3, seed=60 + d)
    return _gen(dict(n_a=5, n_c=3, n_d=5), dict(n_b=5, n_c=3, n_d=5), seed=50 + d, m=m)


def big():
    """200 000 point landmarks, 3 entries of 1 500 + 200 tuples, 60 landmarks named from two entries"""
    m = LM.synthetic_map(n_kf=60, n_pt=200_000, n_ls=3000, seed=77, max_obs=4)
    pt = dict(n_a=400, n_b=400, n_c=300, n_d=400)
    return _gen([pt, dict(pt, n_a=370, n_shared=30), dict(pt, n_a=370, n_shared=30)], dict(n_a=50, n_b=50, n_c=50, n_d=50),
                entries=((3, 50, 1), (5, 53, 1), (8, 56, 1)), seed=9, m=m)


_PT = dict(n_a=30, n_b=30, n_c=20, n_d=20)
_LS = dict(n_a=8, n_b=8, n_c=6, n_d=8)

CASES = {
    "no_events": lambda: _gen({}, {}),
    "flag_zero_entry": lambda: _gen(dict(n_a=10, n_b=10, n_c=10, n_d=10), dict(n_a=3, n_b=3, n_c=3, n_d=3),
                                    entries=((3, 30, 1), (5, 33, 0), (8, 36, 1))),
    "null_kind": lambda: _gen(_PT, None),
    "only_a": lambda: _gen(dict(n_a=100), dict(n_a=30)),
    "only_b": lambda: _gen(dict(n_b=100), dict(n_b=30)),
    "only_c": lambda: _gen(dict(n_c=100), dict(n_c=30)),
    "only_d": lambda: _gen(dict(n_d=100), dict(n_d=30)),
    "three_entries": lambda: _gen(_PT, _LS, entries=ENTRIES),
    "mixed": mixed,
    "self_fuse": lambda: _gen(dict(n_self=5, n_d=10), dict(n_self=3, n_d=4)),
    "empty_lists": lambda: _gen(dict(n_empty=5, n_d=10), dict(n_empty=3, n_d=4)),
    "same_feature": same_feature,
    "dead_then_named": dead_then_named,
    "nested": nested,
    "grown_then_fused": grown_then_fused,
    "diagonal": diagonal,
    "level_limit": lambda: chain(L),
    "level_over": lambda: chain(L + 1),
    **{f"tile_events_{d:+d}": (lambda d=d: tile_events(d)) for d in (-1, 0, 1)},
    **{f"tile_landmarks_{d:+d}": (lambda d=d: tile_landmarks(d)) for d in (-1, 0, 1)},
}

# the branches (tests/lc_fuse_ref.py: BRANCHES) each case exists for: taken at least 3 times
REACHES = {
    "flag_zero_entry": ("flag_zero", "a.act", "d.act"),
    "only_a": ("a.act",),
    "only_b": ("b.act",),
    "only_c": ("c.act",),
    "only_d": ("d.act",),
    "three_entries": ("a.act", "b.act", "c.act", "d.act"),
    "mixed": ("skip.null_slot", "skip.lm_range", "skip.ldx_range", "skip.self_fuse", "skip.empty_b", "skip.graph_kf_range",
              "a.feat_null", "b.feat_null", "c.feat_null0", "c.feat_null1", "d.feat_null", "a.lm_null", "b.lm_null", "d.lm_null",
              "a.act", "b.act", "c.act", "d.act", "level.2"),
    "self_fuse": ("skip.self_fuse",),
    "empty_lists": ("skip.empty_b",),
    "same_feature": ("same_feature",),
    "dead_then_named": ("a.lm_dead", "b.lm_dead", "d.lm_dead"),
    "nested": ("d.on_grown_a", "d.copies_appended"),
    "grown_then_fused": ("d.copies_appended",),
    "diagonal": ("a.diagonal", "b.diagonal"),
    "level_limit": ("level.max",),
}


@functools.lru_cache(maxsize=None)
def run_ref(name):
    """-> (m, lc, (map after, out) or None where the restatement refuses, hits); computed once per case and shared: nobody
    writes to it"""
    import collections

    import lc_fuse_ref as R
    m, lc = (big if name == "big" else CASES[name])()
    hits = collections.Counter()
    try:
        after = R.fuse(m, lc, hits)
    except R.LevelExceeded:
        after = None
    return m, lc, after, hits

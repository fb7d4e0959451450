"""The maps the tests of plslam_lc_correct_image share: test_lc_correct_image_cpu.py shows on each that the two restatements agree
and that it reaches what it is named for, the GPU files run the device on them.  T and G are the kernels' MAP_TILE and
LCI_MAX_GRID, read from the sources: a change of either fails the reach assertions instead of silently un-reaching the path."""
import os
import re

import numpy as np

import lc_correct_image_ref as R
from plslam_amd import local_map as LM
from plslam_amd import map_insert as MI

_CSRC = os.path.join(os.path.dirname(os.path.abspath(LM.__file__)), "csrc")


def _constant(source, pattern):
    with open(os.path.join(_CSRC, source)) as f:
        return int(re.search(pattern, f.read()).group(1))


T = _constant("map_image.hpp", r"constexpr int MAP_TILE = (\d+);")
G = _constant("lc_correct_image.hip", r"constexpr unsigned LCI_MAX_GRID = (\d+);")


def tiles(n):
    return -(-int(n) // T)


def hand_map(nk, points, lines, seed=1):
    """an image from explicit landmarks: per kind a list of (valid, [obs_kf, ...]); no features"""
    rng = np.random.Generator(np.random.PCG64(seed))

    def kind(lms, dl, dv):
        n = len(lms)
        lens = [len(o) for _, o in lms]
        ptr = np.zeros(n + 1, np.int32)
        ptr[1:] = np.cumsum(lens)
        okf = np.array([k for _, o in lms for k in o], np.int32)
        return dict(n=n, valid=np.array([v for v, _ in lms], np.uint8), inlier=np.ones(n, np.uint8), X=rng.uniform(-20.0, 20.0, (n, dl)),
                    obs_ptr=ptr, obs_kf=okf, obs_val=rng.uniform(0.0, 700.0, (okf.size, dv)), feat_ptr=np.zeros(nk + 1, np.int32),
                    feat_idx=np.zeros(0, np.int32))

    return dict(n_map_kf=nk, kf_valid=np.ones(nk, np.uint8), x_kf_w=rng.standard_normal((nk, 6)), row=np.zeros(nk, np.int32),
                points=kind(points, 3, 2), lines=kind(lines, 6, 3))


def length_map(nk, lines_too=True, seed=4):
    """lists of 0, 1, 63, 64 and 65 rows, then one of 300 rows that lies across the first workgroup boundary of the direction pass
    (rows 193 .. 492), then short ones; list i is first seen in slot i mod nk"""
    rng = np.random.Generator(np.random.PCG64(seed))
    lens = [0, 1, 63, 64, 65, 300, 0, 2, 5, 1, 0, 64, 3]
    lms = [(1, [i % nk] * min(ln, 1) + [int(k) for k in rng.integers(0, nk, max(ln - 1, 0))]) for i, ln in enumerate(lens)]
    lms[7] = (0, lms[7][1])                                       # an invalid landmark among them
    return hand_map(nk, lms, lms if lines_too else [], seed)


def decision_map():
    """4 slots; slot 3 anchors nothing.  Points: 0 valid, first seen in 0; 1 INVALID, first seen in 0; 2 valid, first seen in 1;
    3 valid, first observer -1; 4 valid, first observer n_map_kf; 5 valid without observations; 6 valid, first seen in 2, later
    in 3.  The lines are the same."""
    lms = [(1, [0, 1]), (0, [0, 2]), (1, [1, 3]), (1, [-1, 0]), (1, [4, 0]), (1, []), (1, [2, 3])]
    return hand_map(4, lms, lms, seed=9)


def inputs(m, seed):
    """-> T_corr (every slot its own MI._pose), lists (the dir rows alone), med_dir, x_kf_w_new"""
    rng = np.random.Generator(np.random.PCG64(seed))
    nk = m["n_map_kf"]
    T_corr = np.stack([MI._pose(rng) for _ in range(nk)])
    lists = {kind: dict(dir=rng.standard_normal((m[kind]["obs_kf"].size, 3))) for kind in R.KINDS}
    med = {kind: rng.standard_normal((m[kind]["n"], 3)) for kind in R.KINDS}
    return T_corr, lists, med, rng.standard_normal((nk, 6))


def row_landmark(K):
    """per dir row the landmark whose list holds it"""
    return np.repeat(np.arange(K["n"]), np.diff(np.asarray(K["obs_ptr"], np.int64)))


def tile_ends(K):
    """per tile of the direction pass the landmarks of its first and of its last row: what tile_bounds has to find"""
    lm, n_obs = row_landmark(K), int(K["obs_kf"].size)
    first = np.arange(0, n_obs, T)
    return lm[first], lm[np.minimum(first + T, n_obs) - 1]


# ---- a. the depth of the workgroup-wide search -------------------------------------------------------------------------------------
DEPTH_SIZES = (T - 1, T, T + 1, T * T - 1, T * T, T * T + 1)
DEPTH_ROUNDS = (1, 1, 2, 2, 2, 3)
DEPTH_WITH_LINES = T * T + 1
DEPTH_NK = 5


def search_rounds(n, j):
    """tile_bounds' rounds for a row of landmark j among n, restated: a round cuts [lo, lo + len) into pieces of
    step = ceil(len / T) and keeps the piece that holds j, len = min(step, what is left of the range).
    -> [(lo, len, step) as each round finds them], short: a round kept a last piece shorter than its step"""
    lo, ln, out, short = 0, int(n), [], False
    while ln > 1:
        step = -(-ln // T)
        out.append((lo, ln, step))
        end = lo + ln
        lo += (j - lo) // step * step
        short |= end - lo < step
        ln = min(step, end - lo)
    assert lo == j or n == 0
    return out, short


def depth_map(n, ends_empty, seed=40):
    """n point landmarks (DEPTH_WITH_LINES: as many lines), all valid, with lists of 0, 1, 1, 1, 2 or 3 rows, so rows and landmarks
    do not coincide; the first and the last landmark are empty or not as `ends_empty` says, the second and the last but one always
    hold rows; first observers cycle over the 5 slots"""
    rng = np.random.Generator(np.random.PCG64(seed + n + ends_empty))

    def kind(n, dl, dv):
        lens = rng.choice(np.array([0, 1, 1, 1, 2, 3]), n)
        lens[[1, -2]] = 2
        lens[[0, -1]] = 0 if ends_empty else 3
        ptr = np.zeros(n + 1, np.int32)
        ptr[1:] = np.cumsum(lens)
        okf = rng.integers(0, DEPTH_NK, int(ptr[-1])).astype(np.int32)
        has = lens > 0
        okf[ptr[:-1][has]] = (np.arange(n) % DEPTH_NK)[has]
        return dict(n=n, valid=np.ones(n, np.uint8), inlier=np.ones(n, np.uint8), X=rng.uniform(-20.0, 20.0, (n, dl)), obs_ptr=ptr,
                    obs_kf=okf, obs_val=rng.uniform(0.0, 700.0, (okf.size, dv)), feat_ptr=np.zeros(DEPTH_NK + 1, np.int32),
                    feat_idx=np.zeros(0, np.int32))

    n_ls = n if n == DEPTH_WITH_LINES else 0
    empty = hand_map(DEPTH_NK, [], [], seed)
    return dict(empty, points=kind(n, 3, 2), lines=kind(n_ls, 6, 3) if n_ls else empty["lines"])


def depth_reach(m, n):
    """what depth_map(n, ...) has to reach, from its own arrays"""
    want = DEPTH_ROUNDS[DEPTH_SIZES.index(n)]
    for kind in R.KINDS if n == DEPTH_WITH_LINES else ("points",):
        K = m[kind]
        assert K["n"] == n and K["obs_kf"].size != n and (np.diff(K["obs_ptr"]) >= 0).all()
        runs = [search_rounds(n, int(j)) for ends in tile_ends(K) for j in ends]
        assert max(len(r) for r, _ in runs) == want, (kind, n)
        assert max(len(search_rounds(n, j)[0]) for j in range(0, n, max(n // 997, 1))) == want      # no landmark needs more
        if n == T * T + 1:                                        # the short last piece: T pieces of T + 1, one of 2 is left
            last, short = search_rounds(n, int(tile_ends(K)[1][-1]))
            assert short and last[1][1] == 2 < last[0][2] == T + 1, (kind, last)
        assert sorted(set(K["obs_kf"][K["obs_ptr"][:-1][np.diff(K["obs_ptr"]) > 0]].tolist())) == list(range(DEPTH_NK))


# ---- b. tiles that lie inside one list ------------------------------------------------------------------------------------------------
INSIDE_NK = 3
INSIDE_INVALID = 600


def inside_map(seed=50):
    """3 slots; list i is first seen in slot i mod 3.  An empty landmark; lists of 2T - 1 rows (from row 0: it starts on a tile's
    first row), 1, 2T (tiles 2 and 3 exactly: it ends on a tile's last row), 2T + 1 (tile 5 strictly inside) and T - 1 rows; T + 1
    empty landmarks; 1000 rows from row 7T; T + 1 empty landmarks; 3 rows; an INVALID landmark with 600 rows; 3T + 1 rows; 5 rows;
    three empty landmarks."""
    rng = np.random.Generator(np.random.PCG64(seed))
    lens = [0, 2 * T - 1, 1, 2 * T, 2 * T + 1, T - 1] + [0] * (T + 1) + [1000] + [0] * (T + 1) + [3, INSIDE_INVALID, 3 * T + 1, 5, 0, 0, 0]
    lms = [(int(ln != INSIDE_INVALID), [i % INSIDE_NK] * min(ln, 1) + rng.integers(0, INSIDE_NK, max(ln - 1, 0)).tolist())
           for i, ln in enumerate(lens)]
    return hand_map(INSIDE_NK, lms, lms[:8], seed)


def inside_reach(m):
    """the placement inside_map promises, from obs_ptr"""
    K = m["points"]
    ptr, valid = np.asarray(K["obs_ptr"], np.int64), K["valid"]
    b, e, lens = ptr[:-1], ptr[1:], np.diff(ptr)
    assert m["n_map_kf"] == INSIDE_NK and {511, 512, 513, 1000, 3 * T + 1} <= set(lens.tolist())
    long_ = lens >= 2 * T - 1                                     # a list that can hold a whole tile
    assert (long_ & (b % T == 0)).any() and (long_ & (e % T == 0)).any()
    first, last = tile_ends(K)
    row0 = np.arange(first.size) * T
    whole = (first == last) & (row0 + T <= K["obs_kf"].size)      # a tile of T rows inside one list: jb[0] == jb[1]
    strictly = whole & (b[first] < row0) & (row0 + T < e[first])
    assert whole.sum() >= 10 and strictly.any() and (whole & (valid[first] == 0)).any() and (whole & (valid[first] == 1)).any()
    for j in np.flatnonzero(lens == 1000).tolist() + np.flatnonzero(lens == INSIDE_INVALID).tolist():
        assert whole[first == j].any(), j
    j = int(np.flatnonzero(lens == 1000)[0])                      # T + 1 empty landmarks directly before and directly after
    assert (lens[j - T - 1:j] == 0).all() and (lens[j + 1:j + T + 2] == 0).all() and lens[j - T - 2] > 0 and lens[j + T + 2] > 0
    assert lens[0] == 0 and lens[-1] == 0 and lens[-2] == 0 and valid[lens == INSIDE_INVALID].tolist() == [0]
    assert len({int(K["obs_kf"][b[i]]) for i in np.flatnonzero(long_)}) == INSIDE_NK
    return int(whole.sum())


# ---- c. the walk -------------------------------------------------------------------------------------------------------------------------
WALK_A, WALK_B, WALK_C = 0, 1, 2


def walk_map(seed=60):
    """More tiles than workgroups in both passes: G T + 5 points, 300 lines and T + 3 slots, lists of up to 4 rows.  The first
    observers are overwritten: a point in the first G tiles of the landmark pass is first seen in slot A where its list starts in
    the first G tiles of the direction pass and in slot C where it starts beyond; the points of the last tile are first seen in
    slot B.  The first half of the lines is first seen in slot A, the second in slot B."""
    m = LM.synthetic_map(n_kf=T + 3, n_pt=G * T + 5, n_ls=300, seed=seed, max_obs=4)
    for kind in R.KINDS:
        K = m[kind]
        ptr, n = np.asarray(K["obs_ptr"], np.int64), K["n"]
        j = np.arange(n)
        slot = np.where(j >= G * T, WALK_B, np.where(ptr[:-1] >= G * T, WALK_C, WALK_A)) if kind == "points" else \
            np.where(j >= n // 2, WALK_B, WALK_A)
        has = np.diff(ptr) > 0
        K["obs_kf"] = K["obs_kf"].copy()
        K["obs_kf"][ptr[:-1][has]] = slot[has]
    return m


WALK_PATTERNS = ("every slot", "slot A and half the others", "slot B only", "slots B and C", "no slot")


def walk_corrected(pattern, nk=T + 3):
    k = np.arange(nk)
    return {"every slot": k >= 0, "slot A and half the others": k % 2 == 0, "slot B only": k == WALK_B,
            "slots B and C": (k == WALK_B) | (k == WALK_C), "no slot": k < 0}[pattern]


def first_observer(K):
    """per landmark its first observer, -1 where its list is empty"""
    ptr = np.asarray(K["obs_ptr"], np.int64)
    first = np.full(K["n"], -1, np.int64)
    has = np.diff(ptr) > 0
    first[has] = K["obs_kf"][ptr[:-1][has]]
    return first


def walk_reach(m):
    """what walk_map has to reach, from the image: -> (tiles of the landmark pass, tiles of the direction pass)"""
    P, L, nk = m["points"], m["lines"], m["n_map_kf"]
    tp, tl, tk = tiles(P["n"]), tiles(L["n"]), tiles(nk)
    dp, dl = tiles(P["obs_kf"].size), tiles(L["obs_kf"].size)
    # the landmark pass: more tiles than workgroups; every line tile, both slot tiles and the points of slot B lie beyond the
    # first G, so they are reached only by walking
    assert tp > G and tl >= 2 and tk == 2
    # the direction pass: some workgroups take three tiles, some two
    assert P["obs_kf"].size > 2 * G * T and 2 * G < dp + dl < 3 * G and (dp + dl) % G != 0 and dp >= 2 * G
    for n in (P["n"], L["n"], nk, P["obs_kf"].size, L["obs_kf"].size):
        assert n % T != 0                                         # the last tile of each array is partial
    fp, fl, valid = first_observer(P), first_observer(L), P["valid"] == 1
    lm_tile = np.arange(P["n"]) // T
    assert set(fp[lm_tile < G].tolist()) == {-1, WALK_A, WALK_C} and set(fp[lm_tile >= G].tolist()) <= {-1, WALK_B}
    assert ((fp == WALK_B) & valid).any() and set(fl.tolist()) == {-1, WALK_A, WALK_B}
    assert ((fl == WALK_A) & (L["valid"] == 1)).any() and ((fl == WALK_B) & (L["valid"] == 1)).any()
    # slots A and C: every tile of the landmark pass's first visit has a point to move; slot B: none has
    assert (np.bincount(lm_tile[valid & (fp >= 0)], minlength=tp)[:G] > 0).all()
    # the direction pass: the rows of the first visit are slot A's alone and every tile of it has one to move; every tile of the
    # second visit has a row of slot C and the first visit has none; the rows of slot B lie in tiles of the third visit (the
    # lines' rows come after the points': third visit as well)
    row_lm = row_landmark(P)
    row_first, row_tile, row_valid = fp[row_lm], np.arange(row_lm.size) // T, valid[row_lm]
    assert set(row_first[row_tile < G].tolist()) == {WALK_A}
    assert (np.bincount(row_tile[(row_first == WALK_A) & row_valid], minlength=dp)[:G] > 0).all()
    assert (np.bincount(row_tile[(row_first == WALK_C) & row_valid], minlength=dp)[G:2 * G] > 0).all()
    b_tiles = np.unique(row_tile[(row_first == WALK_B) & row_valid])
    assert b_tiles.size and (b_tiles >= 2 * G).all()
    return tp + tl + tk, dp + dl

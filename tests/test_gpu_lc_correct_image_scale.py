"""plslam_lc_correct_image (K105-K107) where test_gpu_lc_correct_image.py does not reach: the workgroup-wide search of tile_bounds
at one, two and three rounds and with a short last piece, tiles of the direction pass that lie inside one list, and maps with more
tiles than LCI_MAX_GRID workgroups, so that a workgroup walks from tile to tile.  Every comparison is bitwise against the
vectorised restatement (lc_correct_image_ref.correct_image_fast, which test_lc_correct_image_cpu.py pins to the loop), with dir,
med_dir and x_kf_w carried and every slot its own T_corr; every map shows by arithmetic on its own arrays
(lc_correct_image_cases.*_reach) that it reaches what it is named for."""
import numpy as np
import pytest

import lc_correct_image_cases as CS
import lc_correct_image_ref as R
import test_gpu_lc_correct_image as G
from plslam_amd import local_map as LM

pytestmark = pytest.mark.gpu


class _Dirs:
    """the dir rows alone on the device with the ptr() and host() of a DeviceMapLists: the call reads nothing else of the lists"""

    def __init__(self, lists, dev):
        import torch
        self._t = {f"{k}.dir": (torch.from_numpy(np.ascontiguousarray(lists[k]["dir"]) if lists[k]["dir"].size else np.zeros((1, 3))).to(dev),
                                lists[k]["dir"].shape[0]) for k in R.KINDS}

    def ptr(self, name):
        return self._t[name][0].data_ptr()

    def host(self, name):
        t, n = self._t[name]
        return t.cpu().numpy()[:n]


class _Device(G._Device):
    def __init__(self, ctx, m, lists, med):
        import torch
        super().__init__(ctx, m, None, med)
        self.lists = _Dirs(lists, torch.device("cuda", ctx.device))


def _run(ctx, m, given, corrected, what):
    """a fresh upload, the call, the restatement -> the counts"""
    T_corr, lists, med, x_new = given
    co = np.asarray(corrected, bool)
    d = _Device(ctx, m, lists, med)
    counts = d.correct(T_corr, co, x_new)
    want = R.correct_image_fast(m, T_corr, co, x_new, lists, med)
    G._same(d.state(), want, what)
    assert counts == want["counts"], (what, counts, want["counts"])
    return counts


def _counts_of(m, corrected):
    """the four counts from the image alone: the valid landmarks first seen in a corrected slot, and the rows of their lists"""
    out, co = {}, np.asarray(corrected, bool)
    for kind, tag in zip(R.KINDS, ("pt", "ls")):
        K = m[kind]
        first = CS.first_observer(K)
        moved = (K["valid"] == 1) & (first >= 0) & co[np.maximum(first, 0)]
        out[f"n_{tag}"], out[f"n_{tag}_dirs"] = int(moved.sum()), int(np.diff(K["obs_ptr"])[moved].sum())
    return out


def test_the_constants_the_cases_are_built_around_are_the_kernels():
    assert CS.T == LM.LOOKBACK_TILE == G.T and (CS.T, CS.G) == (256, 2048)


# ---- a. one, two and three rounds of tile_bounds ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ends_empty", [False, True])
@pytest.mark.parametrize("n", CS.DEPTH_SIZES)
def test_the_search_at_every_depth(ctx, n, ends_empty):
    """A bound that is off makes last_not_above return a landmark whose list does not hold the row: the row stays while the
    restatement moves it (every slot corrected), or takes a neighbour's decision (alternate slots)."""
    m = CS.depth_map(n, ends_empty)
    CS.depth_reach(m, n)
    given = CS.inputs(m, 80 + n % 7)
    for corrected in ([1, 1, 1, 1, 1], [1, 0, 1, 0, 1]):
        c = _run(ctx, m, given, corrected, (n, ends_empty, corrected))
        assert c == _counts_of(m, corrected) and c["n_pt"] > n // 3 and c["n_pt_dirs"] > c["n_pt"]
        assert (c["n_ls"] > n // 3 and c["n_ls_dirs"] > c["n_ls"]) if n == CS.DEPTH_WITH_LINES else c["n_ls"] == c["n_ls_dirs"] == 0


# ---- b. tiles inside one list -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("corrected", [[1, 1, 1], [1, 0, 0], [0, 0, 1]])
def test_tiles_that_lie_inside_one_list(ctx, corrected):
    m = CS.inside_map()
    assert CS.inside_reach(m) == 12
    c = _run(ctx, m, CS.inputs(m, 90), corrected, corrected)
    assert c == _counts_of(m, corrected) and c["n_pt_dirs"] >= 2 * CS.T and c["n_ls_dirs"] >= CS.T
    assert c["n_pt_dirs"] <= np.diff(m["points"]["obs_ptr"]).sum() - CS.INSIDE_INVALID       # the invalid landmark's rows stay


# ---- c. the walk ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walk():
    m = CS.walk_map()
    return m, CS.walk_reach(m), CS.inputs(m, 61)


@pytest.mark.parametrize("pattern", CS.WALK_PATTERNS)
def test_more_tiles_than_workgroups(ctx, walk, pattern):
    """every slot: all tiles busy.  Slot A and half the others (slot C among them): every workgroup's first tile is busy in both
    passes, the tiles of slot B are idle.  Slot B only: a workgroup is idle on every visit before the one that holds slot B's
    rows, and leaves tile_xform early there.  Slots B and C: every workgroup of the direction pass is idle on its first visit and
    busy on its second.  No slot: nothing changes."""
    m, (lm_tiles, dir_tiles), given = walk
    assert lm_tiles > CS.G and 2 * CS.G < dir_tiles < 3 * CS.G
    co = CS.walk_corrected(pattern, m["n_map_kf"])
    c = _run(ctx, m, given, co, pattern)
    assert c == _counts_of(m, co)
    n_pt_rows = int(m["points"]["obs_kf"].size)
    if pattern == "every slot":
        assert c["n_pt"] > 9 * CS.G * CS.T // 10 and c["n_pt_dirs"] > 2 * CS.G * CS.T and c["n_ls"] > 250
    elif pattern == "slot A and half the others":
        assert c["n_pt"] > 9 * CS.G * CS.T // 10 and 0 < c["n_ls"] < 160
    elif pattern == "slot B only":
        assert 0 < c["n_pt"] <= 5 and 0 < c["n_pt_dirs"] <= 20 and 0 < c["n_ls"] < 160 and c["n_ls_dirs"] > 0
    elif pattern == "slots B and C":
        assert 0 < c["n_pt_dirs"] <= n_pt_rows - CS.G * CS.T + 4 and c["n_pt_dirs"] > CS.G * CS.T // 2
    else:
        assert c == dict(n_pt=0, n_ls=0, n_pt_dirs=0, n_ls_dirs=0)

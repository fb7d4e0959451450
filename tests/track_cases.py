"""Hand-made tables for the tracker's row kernels (tests/test_track_cpu.py pins the two restatements on them,
tests/test_gpu_track.py runs them on the device): per kind a match table, the two stereo tables, disparities and geometry with
the edge entries placed by rule, not drawn."""
import numpy as np

N_PREV = (0, 1, 63, 64, 65, 255, 256, 257, 513)       # around one wave, one 256-row chunk, two chunks
MODES = ("all", "none", "alt", "edges")
CAM = dict(fx=458.654, fy=457.296, cx=367.215, cy=248.375, b=0.110)


def kind_tables(rng, n_prev, n_curr, mode, lines):
    """(m, st_prev, disp, f_prev, st_curr, f_curr) of one kind.  mode: "all" every row kept (a permutation-like table into
    curr), "none" (every entry -1), "alt" every other row kept, "edges": by i1 % 8 -- 0, 5, 7 kept, 1 entry -1, 2 entry n_curr
    (the first past the end), 3 entry 2^31 - 1, 4 stereo -1 in prev, 6 stereo -1 in curr (its i2 is used by no kept row), and the
    first kept row carries a zero disparity, the second kept row points at a zero-length segment (lines)."""
    w = 4 if lines else 2
    f_prev = rng.uniform(5, 700, (n_prev, w)).astype(np.float32)
    f_curr = rng.uniform(5, 700, (n_curr, w)).astype(np.float32)
    disp = rng.uniform(1.0, 40.0, (n_prev, 2) if lines else n_prev)
    st_prev = rng.integers(0, 1000, n_prev).astype(np.int32)
    st_curr = rng.integers(0, 1000, n_curr).astype(np.int32)
    m = (np.arange(n_prev) * 7 + 3) % max(n_curr, 1) if n_curr else np.full(n_prev, -1)
    m = m.astype(np.int32)
    i = np.arange(n_prev)
    if mode == "none":
        m[:] = -1
    elif mode == "alt":
        m[i % 2 == 1] = -1
    elif mode == "edges":
        m[i % 8 == 1] = -1
        m[i % 8 == 2] = n_curr
        m[i % 8 == 3] = 2 ** 31 - 1
        st_prev[i % 8 == 4] = -1
        if n_curr >= 2:
            m[i % 8 == 6] = n_curr - 1                # only these rows point at the last row of curr, whose stereo entry is -1
            other = (i % 8 != 6) & (m == n_curr - 1)
            m[other] = 0
            st_curr[n_curr - 1] = -1
        kept = [k for k in range(n_prev) if 0 <= m[k] < n_curr and st_prev[k] >= 0 and st_curr[m[k]] >= 0]
        if kept:
            if lines:
                disp[kept[0], 1] = 0.0
            else:
                disp[kept[0]] = 0.0
        if lines and len(kept) > 1:
            f_curr[m[kept[1]], 2:] = f_curr[m[kept[1]], :2]
    return m, st_prev, disp, f_prev, st_curr, f_curr


def pair(seed, n_pt, n_ls, mode, n_pt_curr=None, n_ls_curr=None):
    rng = np.random.Generator(np.random.PCG64(seed))
    n_pt_curr = n_pt + 3 if n_pt_curr is None else n_pt_curr
    n_ls_curr = max(n_ls - 2, 1) if n_ls_curr is None else n_ls_curr
    p = kind_tables(rng, n_pt, n_pt_curr, mode, False)
    q = kind_tables(rng, n_ls, n_ls_curr, mode, True)
    return dict(m_pt=p[0], st_pt_prev=p[1], disp_pt_prev=p[2], kp_prev=p[3], st_pt_curr=p[4], kp_curr=p[5],
                m_ls=q[0], st_ls_prev=q[1], disp_ls_prev=q[2], seg_prev=q[3], st_ls_curr=q[4], seg_curr=q[5])


def edge_pairs():
    """Every (n_prev, mode) with both kinds (lines at another size of the list), then points only and lines only at 257"""
    out, names = [], []
    for k, n in enumerate(N_PREV):
        for j, mode in enumerate(MODES):
            out.append(pair(100 * k + j, n, N_PREV[(k + 3) % len(N_PREV)], mode))
            names.append(f"n{n}-{mode}")
    for j, mode in enumerate(MODES):
        out.append(pair(9000 + j, 257, 0, mode, n_ls_curr=0))
        names.append(f"points-only-{mode}")
        out.append(pair(9100 + j, 0, 257, mode, n_pt_curr=0))
        names.append(f"lines-only-{mode}")
    return names, out


def scene_tables(p):
    """A scene pair (plslam_amd.track.track_pair_scene) as the tracker's input, from its TRUE tables: no matcher, no gates"""
    from plslam_amd import track as TR
    dp, dl = TR.true_disparities(p, "p")
    return dict(m_pt=p["m_pt"], st_pt_prev=p["st_pt_prev"], disp_pt_prev=dp, kp_prev=p["kp_pl"], st_pt_curr=p["st_pt_curr"],
                kp_curr=p["kp_cl"], m_ls=p["m_ls"], st_ls_prev=p["st_ls_prev"], disp_ls_prev=dl, seg_prev=p["seg_pl"],
                st_ls_curr=p["st_ls_curr"], seg_curr=p["seg_cl"])


# ---- the scenes of the pose tests: six pairs, one without lines and one without points; their tables come from the truth
# (pose_pairs) or from descriptors through the matcher and the stereo gates (chain_pairs: the oracle's, the device must
# produce the same).  Built once per process.
POSE_SEED, POSE_SIZES = 21, [(300, 60), (300, 60), (300, 0), (300, 60), (0, 60), (300, 60)]
CHAIN_SEED, CHAIN_SIZES = 22, [(300, 60), (200, 40), (300, 60)]
NNR, MUTUAL = 0.75, True
_cache = {}


def scene_cam():
    from plslam_amd import track as TR
    return TR.SCENE_CAM


def gates():
    from plslam_amd import synth
    return dict(synth.KITTI_GATES)


def pose_pairs():
    from plslam_amd import track as TR
    if "pose" not in _cache:
        _cache["pose"] = [scene_tables(p) for p in TR.track_scene(POSE_SEED, len(POSE_SIZES), sizes=POSE_SIZES)]
    return _cache["pose"]


def chain_scene():
    from plslam_amd import track as TR
    if "chain_scene" not in _cache:
        _cache["chain_scene"] = TR.track_scene(CHAIN_SEED, len(CHAIN_SIZES), sizes=CHAIN_SIZES)
    return _cache["chain_scene"]


def chain_pairs():
    """The tracker's input of every pair of chain_scene() as the oracle's matcher and gates make it from descriptors and
    geometry, plus the tables the device's match plan must reproduce: (pairs, tables) with tables[b] a dict of
    "pp", "cc" (L <-> R of prev / curr), "pc" (prev <-> curr), each (points table, lines table)"""
    from oracle import oracle as O
    if "chain" not in _cache:
        g, pairs, tables = gates(), [], []
        for p in chain_scene():
            m = {k: (O.match(p[f"pdesc_{a}"], p[f"pdesc_{b}"], NNR, MUTUAL)[0], O.match(p[f"ldesc_{a}"], p[f"ldesc_{b}"], NNR, MUTUAL)[0])
                 for k, a, b in (("pp", "pl", "pr"), ("cc", "cl", "cr"), ("pc", "pl", "cl"))}
            with np.errstate(all="ignore"):
                sp = O.stereo_point_gate(m["pp"][0], p["kp_pl"], p["kp_pr"], g["max_dist_epip"], g["min_disp"])
                sc = O.stereo_point_gate(m["cc"][0], p["kp_cl"], p["kp_cr"], g["max_dist_epip"], g["min_disp"])
                lp = O.stereo_line_gate(m["pp"][1], p["seg_pl"], p["seg_pr"], g["min_disp"], g["line_horiz_th"], g["stereo_overlap_th"], g["ls_min_disp_ratio"])
                lc = O.stereo_line_gate(m["cc"][1], p["seg_cl"], p["seg_cr"], g["min_disp"], g["line_horiz_th"], g["stereo_overlap_th"], g["ls_min_disp_ratio"])
            pairs.append(dict(m_pt=m["pc"][0], st_pt_prev=sp[0], disp_pt_prev=sp[1], kp_prev=p["kp_pl"], st_pt_curr=sc[0], kp_curr=p["kp_cl"],
                              m_ls=m["pc"][1], st_ls_prev=lp[0], disp_ls_prev=lp[1], seg_prev=p["seg_pl"], st_ls_curr=lc[0], seg_curr=p["seg_cl"]))
            tables.append(m)
        _cache["chain"] = (pairs, tables)
    return _cache["chain"]


def gn_references(which):
    """per pair of pose_pairs() / chain_pairs(): (track_ref rows, lc_ref.relpose_robust_gn on them, params dict)"""
    import lc_ref
    import track_ref
    from oracle import oracle as O
    from plslam_amd import loop_closure as LC
    if ("gn", which) not in _cache:
        cam = scene_cam()
        prm = LC.params_dict(LC.params(cam=cam))
        pairs = pose_pairs() if which == "pose" else chain_pairs()[0]
        out = []
        for p in pairs:
            r = track_ref.rows_seq(cam, p)
            with np.errstate(all="ignore"):
                out.append((r, lc_ref.relpose_robust_gn(prm, O.make_cam(**cam), r["P"], r["pl_obs"], r["sPeP"], r["le_obs"]), prm))
        _cache[("gn", which)] = out
    return _cache[("gn", which)]


def margins(ref, prm):
    """What a comparison of masks and decisions needs of a reference (tests/test_gpu_loop_closure.py::_margins): no residual
    within 0.05 px of sqrt(7.815) at the outlier pass, no decision value within 1 % of its threshold"""
    import lc_ref
    for r in ref["res_at_outlier_pass"]:
        r = r[np.isfinite(r)]
        assert r.size == 0 or np.min(np.abs(r - lc_ref.CHI)) >= 0.05, "a residual sits on the outlier threshold"
    for v, th in ((ref["e"], prm["lc_res"]), (ref["cov_eig"], prm["lc_unc"]), (ref["t"], prm["lc_trs"]), (ref["r"], prm["lc_rot"])):
        if np.isfinite(v):
            assert abs(v - th) >= 0.01 * abs(th), f"{v} is within 1 % of its threshold {th}"


def small_pairs(B, seed=5):
    """B pairs with n_prev <= 8 per kind; empty pairs at the start, in the middle and at the end"""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for b in range(B):
        empty = b in (0, B // 2, B - 1)
        n_pt, n_ls = (0, 0) if empty else (int(rng.integers(0, 9)), int(rng.integers(0, 9)))
        out.append(pair(70000 + 31 * seed + b, n_pt, n_ls, ("all", "alt", "edges")[b % 3]))
    return out

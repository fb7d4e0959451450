"""The local BA's Schur step (plslam_amd/csrc/lba_schur.hip K19-K24, schur_landmark in lba_blocks_dev.hpp) twice over, for
tests/test_lba_schur_cases_cpu.py and tests/test_gpu_lba_schur_edges.py.  numpy only.

(a) restate / restate_backsub: a sequential float64 restatement IN THE DEVICE'S OPERATION ORDER.  The library is built with
    -ffp-contract=off and the step has no atomics and nothing scheduling-dependent, so the device's words are these words.
    Vectorised across landmarks, pairs, chunks and blocks only -- never across the terms of one sum: no np.sum, @, einsum,
    np.linalg or math.fsum between the markers below.
(b) truth / truth_steps / whole_system: the same quantities in np.longdouble, sums in any order, a landmark's inverse by pivoted
    elimination (gba_dense.solve_long_double).  Shares with (a) only the flags of the landmarks (a) found singular: they are
    dropped.  schur_solve / exact_residual: the long-double Schur route as a solver for any right-hand side and the residual of
    the whole system in rational arithmetic, for the CPU test that sets the two routes against each other.
(c) bounds: what ties (a) to (b), entry by entry.

The lists (build_lists) are a Python mirror of lba_lists.hpp's build_csr / build_schur_pairs in their documented order; the GPU
test shows the mirror equal to plslam_lba_plan_lists."""
from __future__ import annotations

import numpy as np

from gba_dense import LD, solve_long_double

EPS = np.finfo(np.float64).eps
POSE_CHUNK = SCH_CHUNK = 64            # lba_lists.hpp
BACK_WG = 192                          # lba_schur.hip

# The error of the restated Gauss-Jordan inverse (no pivoting) against the long-double inverse, as the largest
#     |Vinv64 - Vinv_ld|_max / (EPS * kappa_j * |Vinv_ld|_max)
# over every landmark of every case of lba_schur_cases.py and every lambda of its table (0 for the full-rank cases included; the
# lambdas the cap drops included too); kappa_j = the 2-norm condition number of the damped block.  test_lba_schur_cases_cpu.py::
# test_the_measurement_of_c_inv repeats the measurement.  The algorithm measured is the one bounded: the factor 4 only covers
# landmarks between the sampled ones.
C_INV_MEASURED = 0.6503               # measured: 0.650256, on wide_baseline at lambda = 10 (a point block)
C_INV = 4 * C_INV_MEASURED


# ---- the lists: lba_lists.hpp ------------------------------------------------------------------------------------------------------
def _csr_by_key(key, nkeys):
    """csr_by_key: the observations by key, list order (a stable counting sort)"""
    key = np.asarray(key, np.int64)
    ptr = np.zeros(nkeys + 1, np.int32)
    ptr[1:] = np.cumsum(np.bincount(key, minlength=nkeys)) if key.size else 0
    return ptr, np.argsort(key, kind="stable").astype(np.int32)


def build_lists(c):
    """what plslam_lba_plan_lists(prepare_schur=True) returns for the columns of case c (the lists and the scalars, not the columns)"""
    nkf, npt, nls = c["nkf"], c["npt"], c["nls"]
    pt_lm, pt_kf, ls_lm, ls_kf = (np.asarray(c[k], np.int32) for k in ("pt_lm", "pt_kf_loc", "ls_lm", "ls_kf_loc"))
    n_pt_obs = pt_lm.size
    pt_ptr, pt_ids = _csr_by_key(pt_lm, npt)
    ls_ptr, ls_ids = _csr_by_key(ls_lm, nls)
    # keyframe lists: points first, then lines (global ids: lines n_pt_obs + o), observations by a fixed keyframe left out
    kf_lists = [[] for _ in range(nkf)]
    for o in range(n_pt_obs):
        if pt_kf[o] >= 0:
            kf_lists[pt_kf[o]].append(o)
    for o in range(ls_lm.size):
        if ls_kf[o] >= 0:
            kf_lists[ls_kf[o]].append(n_pt_obs + o)
    kf_ptr = np.zeros(nkf + 1, np.int32)
    kf_ptr[1:] = np.cumsum([len(x) for x in kf_lists])
    kf_ids = np.array([o for x in kf_lists for o in x], np.int32)
    max_chunks = max([(len(x) + POSE_CHUNK - 1) // POSE_CHUNK for x in kf_lists], default=0)
    # build_schur_pairs: every ordered pair (o1, o2) of observations of ONE landmark by optimised keyframes with kf(o1) <= kf(o2),
    # by block (k1 <= k2, row-major over the upper triangle), landmark order then list order; a block's point pairs, null pairs
    # (0, 0, 0, 2) up to the next chunk boundary when the block has line pairs, then its line pairs
    nblk = nkf * (nkf + 1) // 2
    blk_of = lambda k1, k2: k1 * nkf - k1 * (k1 - 1) // 2 + (k2 - k1)          # noqa: E731
    per = [([], []) for _ in range(nblk)]
    for line, (ptr, ids, kf) in enumerate(((pt_ptr, pt_ids, pt_kf), (ls_ptr, ls_ids, ls_kf))):
        for j in range(ptr.size - 1):
            for i1 in range(ptr[j], ptr[j + 1]):
                o1 = int(ids[i1]); k1 = int(kf[o1])
                if k1 < 0:
                    continue
                for i2 in range(ptr[j], ptr[j + 1]):
                    o2 = int(ids[i2]); k2 = int(kf[o2])
                    if k2 < k1:
                        continue
                    per[blk_of(k1, k2)][line].append((o1, o2, j, line))
    pairs, blk_ptr = [], [0]
    for pt, ls in per:
        room = (len(pt) + SCH_CHUNK - 1) // SCH_CHUNK * SCH_CHUNK if ls else len(pt)
        pairs += pt + [(0, 0, 0, 2)] * (room - len(pt)) + ls
        blk_ptr.append(len(pairs))
    blk_ptr = np.array(blk_ptr, np.int32)
    schur_chunks = int(((np.diff(blk_ptr) + SCH_CHUNK - 1) // SCH_CHUNK).max()) if nblk else 0
    return dict(pt_ptr=pt_ptr, pt_ids=pt_ids, ls_ptr=ls_ptr, ls_ids=ls_ids, kf_ptr=kf_ptr, kf_ids=kf_ids, pt_lm_loc=pt_lm, pt_kf_loc=pt_kf,
                ls_lm_loc=ls_lm, ls_kf_loc=ls_kf, blk_ptr=blk_ptr, pairs=np.array(pairs, np.int32).reshape(-1, 4),
                max_chunks=int(max_chunks), schur_chunks=schur_chunks)


def blocks_of(B):
    """the six block arrays and the dimensions out of a dict as LbaPlan.blocks() returns it"""
    nkf, npt, nls = B["H_pose"].shape[0], B["H_pt"].shape[0], B["H_ls"].shape[0]
    g = B["g"]
    return nkf, npt, nls, g[:6 * nkf].reshape(nkf, 6), g[6 * nkf:6 * nkf + 3 * npt].reshape(npt, 3), g[6 * nkf + 3 * npt:].reshape(nls, 6)


# ==== (a) the restatement: from here to the next marker no sum is left to numpy =====================================================
def restate_landmarks(H, g, lam):
    """schur_landmark<DL> for every landmark at once -> (Vinv (n, DL, DL), t (n, DL), singular (n,) bool)"""
    n, DL = H.shape[0], H.shape[1]
    A, I = np.array(H, np.float64), np.zeros((n, DL, DL))
    for a in range(DL):
        h = H[:, a, a]
        A[:, a, a] = h + lam * h
        I[:, a, a] = 1.0
    ok = np.ones(n, bool)
    for c in range(DL):
        piv = A[:, c, c].copy()
        pos = piv > 0.0
        ok &= pos
        ip = 1.0 / np.where(pos, piv, 1.0)
        for b in range(DL):
            A[:, c, b] = A[:, c, b] * ip
            I[:, c, b] = I[:, c, b] * ip
        for a in range(DL):
            if a == c:
                continue
            f = A[:, a, c].copy()
            for b in range(DL):
                A[:, a, b] = A[:, a, b] - f * A[:, c, b]
                I[:, a, b] = I[:, a, b] - f * I[:, c, b]
    V = np.where(ok[:, None, None], I, 0.0)
    t = np.zeros((n, DL))
    for a in range(DL):
        acc = np.zeros(n)
        for b in range(DL):
            acc = acc + V[:, a, b] * g[:, b]
        t[:, a] = acc
    return V, t, ~ok


def restate_pair_blocks(W1, W2, V):
    """schur_pair_product<DL>: entry (a, b) of W1^T Vinv W2 for every pair at once; W (n, DL, 6), V (n, DL, DL) -> (n, 6, 6)"""
    n, DL = V.shape[0], V.shape[1]
    out = np.zeros((n, 6, 6))
    for b in range(6):
        u = []
        for x in range(DL):
            t = np.zeros(n)
            for y in range(DL):
                t = t + V[:, x, y] * W2[:, y, b]
            u.append(t)
        for a in range(6):
            s = np.zeros(n)
            for x in range(DL):
                s = s + W1[:, x, a] * u[x]
            out[:, a, b] = s
    return out


def _two_level(ptr, terms, chunk):
    """list k = terms[ptr[k] : ptr[k + 1]]: chunks of `chunk` terms added sequentially in list order from 0.0, then the chunk
    partials in chunk order from 0.0 -> one sum per list (all lists advance together: term by term, chunk by chunk)"""
    ptr = np.asarray(ptr, np.int64)
    nlist = ptr.size - 1
    total = np.zeros((nlist,) + terms.shape[1:])
    if nlist == 0:
        return total
    nch = (np.diff(ptr) + chunk - 1) // chunk
    for c in range(int(nch.max()) if nch.size else 0):
        ks = np.flatnonzero(nch > c)
        beg = ptr[ks] + c * chunk
        n = np.minimum(chunk, ptr[ks + 1] - beg)
        part = np.zeros((ks.size,) + terms.shape[1:])
        for i in range(int(n.max())):
            m = n > i
            part[m] = part[m] + terms[beg[m] + i]
        total[ks] = total[ks] + part
    return total


def restate(B, lists, lam, sch_chunk=SCH_CHUNK):
    """K19-K22 and K24 on the blocks B (LbaPlan.blocks()) and the lists (LbaPlan.lists(prepare_schur=True) or build_lists)
    -> dict(Vp, tp, Vl, tl, sing_pt, sing_ls, n_singular, S, b, diag_max).  (sch_chunk: for the CPU test's mutants only)"""
    nkf, npt, nls, g_pose, g_pt, g_ls = blocks_of(B)
    Vp, tp, sing_pt = restate_landmarks(B["H_pt"], g_pt, lam)
    Vl, tl, sing_ls = restate_landmarks(B["H_ls"], g_ls, lam)
    pairs = lists["pairs"]
    terms = np.zeros((pairs.shape[0], 6, 6))                                   # a null pair contributes 0.0
    for line, W, V in ((0, B["W_pt"], Vp), (1, B["W_ls"], Vl)):
        m = np.flatnonzero(pairs[:, 3] == line)
        if m.size:
            terms[m] = restate_pair_blocks(W[pairs[m, 0]], W[pairs[m, 1]], V[pairs[m, 2]])
    acc = _two_level(lists["blk_ptr"], terms, sch_chunk)
    n6 = 6 * nkf
    S = np.full((n6, n6), np.nan)
    blk = 0
    for k1 in range(nkf):
        for k2 in range(k1, nkf):
            h = np.zeros((6, 6))
            if k1 == k2:
                h = B["H_pose"][k1].copy()
                for a in range(6):
                    h[a, a] = h[a, a] + lam * h[a, a]
            v = h - acc[blk]
            S[6 * k1:6 * k1 + 6, 6 * k2:6 * k2 + 6] = v
            if k1 != k2:
                S[6 * k2:6 * k2 + 6, 6 * k1:6 * k1 + 6] = v.T                  # the lower triangle is the mirror
            blk += 1
    # b: a term per observation of the keyframe lists (points first, then lines)
    ids = lists["kf_ids"].astype(np.int64)
    n_pt_obs = B["W_pt"].shape[0]
    bt = np.zeros((ids.size, 6))
    ip = np.flatnonzero(ids < n_pt_obs)
    if ip.size:
        o = ids[ip]
        W, t = B["W_pt"][o], tp[lists["pt_lm_loc"][o]]
        for a in range(6):
            bt[ip, a] = W[:, 0, a] * t[:, 0] + W[:, 1, a] * t[:, 1] + W[:, 2, a] * t[:, 2]
    il = np.flatnonzero(ids >= n_pt_obs)
    if il.size:
        o = ids[il] - n_pt_obs
        W, t = B["W_ls"][o], tl[lists["ls_lm_loc"][o]]
        for a in range(6):
            s = np.zeros(il.size)
            for x in range(6):
                s = s + W[:, x, a] * t[:, x]
            bt[il, a] = s
    b = (g_pose - _two_level(lists["kf_ptr"], bt, POSE_CHUNK)).reshape(-1)
    dm = 0.0                                                                   # (a maximum: exact whatever the order)
    for H in (B["H_pose"], B["H_pt"], B["H_ls"]):
        for a in range(H.shape[1]):
            dm = max([dm] + np.abs(H[:, a, a]).tolist())
    return dict(Vp=Vp, tp=tp, Vl=Vl, tl=tl, sing_pt=sing_pt, sing_ls=sing_ls, n_singular=int(np.count_nonzero(sing_pt)) + int(np.count_nonzero(sing_ls)), S=S, b=b,
                diag_max=float(dm))


def _backsub_kind(ptr, ids, kf_loc, W, V, t, dp):
    """schur_backsub_wg<DL> for every landmark at once -> (d (n, DL), the workgroups' sums of squares)"""
    n, DL = V.shape[0], V.shape[1]
    ptr = np.asarray(ptr, np.int64)
    acc = np.zeros((n, DL))
    for i in range(int(np.diff(ptr).max()) if n else 0):
        js = np.flatnonzero(ptr[:-1] + i < ptr[1:])
        o = ids[ptr[js] + i]
        k = kf_loc[o].astype(np.int64)
        js, o, k = js[k >= 0], o[k >= 0], k[k >= 0]                            # a fixed keyframe: no cross block, no step
        for x in range(DL):
            s = np.zeros(js.size)
            for a in range(6):
                s = s + W[o, x, a] * dp[6 * k + a]
            acc[js, x] = acc[js, x] + s
    d = np.zeros((n, DL))
    for x in range(DL):
        s = np.zeros(n)
        for y in range(DL):
            s = s + V[:, x, y] * acc[:, y]
        d[:, x] = t[:, x] - s
    # the 192-lane tree of a workgroup: lane q * DL + x holds d^2 of row x of the workgroup's landmark q, 0.0 past the last one
    nwg = (n * DL + BACK_WG - 1) // BACK_WG
    sh = np.zeros(nwg * BACK_WG)
    sh[:n * DL] = (d * d).reshape(-1)
    sh = sh.reshape(nwg, BACK_WG)
    w = 128
    while w > 0:
        lanes = np.array([i for i in range(w) if i + w < BACK_WG])
        sh[:, lanes] = sh[:, lanes] + sh[:, lanes + w]
        w >>= 1
    return d, sh[:, 0].copy()


def restate_backsub(B, lists, R, dp):
    """K23 for the pose step dp on the landmark inverses R = restate(...) -> (dX_pt, dX_ls, sum of squares as apply_step adds it)"""
    dp = np.asarray(dp, np.float64).reshape(-1)
    dxp, part_p = _backsub_kind(lists["pt_ptr"], lists["pt_ids"], lists["pt_kf_loc"], B["W_pt"], R["Vp"], R["tp"], dp)
    dxl, part_l = _backsub_kind(lists["ls_ptr"], lists["ls_ids"], lists["ls_kf_loc"], B["W_ls"], R["Vl"], R["tl"], dp)
    ss = 0.0
    for p in part_p.tolist() + part_l.tolist():                                # points' workgroups first, in workgroup order
        ss = ss + p
    return dxp, dxl, ss
# ==== end of the restatement =======================================================================================================


# ==== (b) the truth: np.longdouble, any order ======================================================================================
def _inverse_ld(A):
    n = A.shape[0]
    eye = np.eye(n, dtype=LD)
    return np.stack([solve_long_double(A, eye[:, i]) for i in range(n)], axis=1)


def truth_landmarks(H, g, lam, singular):
    """-> (Vinv_ld (n, DL, DL), t_ld (n, DL), kappa (n,)): the inverse of H + lam diag(H) by pivoted elimination in long double and
    the 2-norm condition number of that block; a landmark flagged singular is dropped (zeros, kappa 0)"""
    n, DL = H.shape[0], H.shape[1]
    V, kap = np.zeros((n, DL, DL), LD), np.zeros(n)
    for j in range(n):
        if singular[j]:
            continue
        A = np.array(H[j], LD)
        A[np.diag_indices(DL)] += LD(lam) * np.diag(A)
        V[j] = _inverse_ld(A)
        kap[j] = np.linalg.cond(A.astype(np.float64), 2)
    t = np.einsum("jab,jb->ja", V, np.asarray(g, LD)) if n else np.zeros((0, DL), LD)
    return V, t, kap


def _live_obs(lm, kf_loc, n):
    """per landmark: its observations by optimised keyframes (from the raw columns: no list of the plan is used)"""
    out = [[] for _ in range(n)]
    for o in range(lm.size):
        if kf_loc[o] >= 0:
            out[lm[o]].append(o)
    return out


def truth(B, c, lam, sing_pt, sing_ls):
    """S, b, the landmark inverses and t in long double, and beside them what the bounds need in float64: absS / absb = the sums
    of absolute values T_e (h and g included), kapS / kapb = the same sums with each landmark weighted by its kappa"""
    nkf, npt, nls, g_pose, g_pt, g_ls = blocks_of(B)
    n6 = 6 * nkf
    S, b = np.zeros((n6, n6), LD), np.array(g_pose, LD).reshape(-1)
    for k in range(nkf):
        h = np.array(B["H_pose"][k], LD)
        h[np.diag_indices(6)] += LD(lam) * np.diag(h)
        S[6 * k:6 * k + 6, 6 * k:6 * k + 6] = h
    absS, absb = np.abs(S).astype(np.float64), np.abs(b).astype(np.float64)
    kapS, kapb = np.zeros((n6, n6)), np.zeros(n6)
    out = {}
    for tag, H, g, W, lm, kf, sing in (("p", B["H_pt"], g_pt, B["W_pt"], c["pt_lm"], c["pt_kf_loc"], sing_pt),
                                       ("l", B["H_ls"], g_ls, B["W_ls"], c["ls_lm"], c["ls_kf_loc"], sing_ls)):
        V, t, kap = truth_landmarks(H, g, lam, sing)
        out.update({"V" + tag: V, "t" + tag: t, "kap_" + tag: kap})
        Wl, Wa, Va, ga = np.asarray(W, LD), np.abs(W), np.abs(V).astype(np.float64), np.abs(g)
        for j, obs in enumerate(_live_obs(lm, kf, H.shape[0])):
            if sing[j]:
                continue
            for o1 in obs:
                r = slice(6 * kf[o1], 6 * kf[o1] + 6)
                Y, Ya = Wl[o1].T @ V[j], Wa[o1].T @ Va[j]
                b[r] -= Y @ np.asarray(g[j], LD)
                e = Ya @ ga[j]
                absb[r] += e
                kapb[r] += kap[j] * e
                for o2 in obs:
                    q = slice(6 * kf[o2], 6 * kf[o2] + 6)
                    S[r, q] -= Y @ Wl[o2]
                    e = Ya @ Wa[o2]
                    absS[r, q] += e
                    kapS[r, q] += kap[j] * e
    out.update(S=S, b=b, absS=absS, kapS=kapS, absb=absb, kapb=kapb)
    return out


def truth_steps(B, c, Tr, dp):
    """the landmark steps for the pose step dp in long double -> (dX_pt, dX_ls, sum of squares, absdx_pt, absdx_ls); abs*: the sums
    of absolute values |Vinv| (|g| + sum_o |W_o| |dp|)"""
    nkf, npt, nls, g_pose, g_pt, g_ls = blocks_of(B)
    dp = np.asarray(dp, LD).reshape(-1)
    res = []
    for tag, g, W, lm, kf in (("p", g_pt, B["W_pt"], c["pt_lm"], c["pt_kf_loc"]), ("l", g_ls, B["W_ls"], c["ls_lm"], c["ls_kf_loc"])):
        V = Tr["V" + tag]
        rhs, arhs = np.array(g, LD), np.abs(g).astype(LD)
        live = np.flatnonzero(np.asarray(kf) >= 0)
        if live.size:
            dpo = dp.reshape(nkf, 6)[np.asarray(kf)[live]]
            np.subtract.at(rhs, np.asarray(lm)[live], np.einsum("oxa,oa->ox", np.asarray(W, LD)[live], dpo))
            np.add.at(arhs, np.asarray(lm)[live], np.einsum("oxa,oa->ox", np.abs(W).astype(LD)[live], np.abs(dpo)))
        res.append((np.einsum("jab,jb->ja", V, rhs), np.einsum("jab,jb->ja", np.abs(V), arhs).astype(np.float64)))
    (dxp, ap), (dxl, al) = res
    return dxp, dxl, (dxp * dxp).sum() + (dxl * dxl).sum(), ap, al


def dense_system(B, c, lam):
    """the whole damped system H + lam diag(H), g in long double, from the blocks (the layout of the reference's H: keyframes,
    points, lines)"""
    nkf, npt, nls, g_pose, g_pt, g_ls = blocks_of(B)
    N = 6 * nkf + 3 * npt + 6 * nls
    H = np.zeros((N, N), LD)
    for k in range(nkf):
        H[6 * k:6 * k + 6, 6 * k:6 * k + 6] = B["H_pose"][k]
    for base, DL, Hb, W, lm, kf in ((6 * nkf, 3, B["H_pt"], B["W_pt"], c["pt_lm"], c["pt_kf_loc"]),
                                    (6 * nkf + 3 * npt, 6, B["H_ls"], B["W_ls"], c["ls_lm"], c["ls_kf_loc"])):
        for j in range(Hb.shape[0]):
            H[base + DL * j:base + DL * j + DL, base + DL * j:base + DL * j + DL] = Hb[j]
        for o in range(len(lm)):
            if kf[o] >= 0:
                r, q = slice(base + DL * lm[o], base + DL * lm[o] + DL), slice(6 * kf[o], 6 * kf[o] + 6)
                H[r, q] += np.asarray(W[o], LD)
                H[q, r] += np.asarray(W[o], LD).T
    H[np.diag_indices(N)] += LD(lam) * np.diag(H)
    return H, np.array(B["g"], LD)


def whole_system(B, c, lam, sing_pt, sing_ls):
    """the whole damped system with the dropped landmarks' rows and columns deleted -> (H, g, solve): H, g of the kept unknowns and
    solve(rhs in g's layout) = the solution by solve_long_double in g's layout, zeros for the dropped landmarks; `kept` = the mask"""
    nkf, npt, nls = blocks_of(B)[:3]
    H, g = dense_system(B, c, lam)
    keep = np.concatenate([np.ones(6 * nkf, bool), np.repeat(~sing_pt, 3), np.repeat(~sing_ls, 6)])
    Hk = H[np.ix_(keep, keep)]

    def solve(rhs):
        x = np.zeros(g.size, LD)
        x[keep] = solve_long_double(Hk, np.asarray(rhs, LD)[keep])
        return x
    return Hk, g, solve, keep


def schur_solve(B, c, Tr, rhs):
    """the Schur route in long double for ANY right-hand side (the layout of g): b = r_p - sum_o W_o^T Vinv r_l, S dp = b, then the
    back-substitution -> the whole solution vector; Tr = truth(...) holds S and the landmark inverses"""
    nkf, npt, nls = blocks_of(B)[:3]
    rhs = np.asarray(rhs, LD)
    b = rhs[:6 * nkf].copy().reshape(nkf, 6)
    for tag, base, DL, n, W, lm, kf in (("p", 6 * nkf, 3, npt, B["W_pt"], c["pt_lm"], c["pt_kf_loc"]),
                                        ("l", 6 * nkf + 3 * npt, 6, nls, B["W_ls"], c["ls_lm"], c["ls_kf_loc"])):
        live = np.flatnonzero(np.asarray(kf) >= 0)
        if live.size:
            t = np.einsum("jab,jb->ja", Tr["V" + tag], rhs[base:base + DL * n].reshape(n, DL))
            np.subtract.at(b, np.asarray(kf)[live], np.einsum("oxa,ox->oa", np.asarray(W, LD)[live], t[np.asarray(lm)[live]]))
    dp = solve_long_double(Tr["S"], b.reshape(-1))
    dxp, dxl = truth_steps(dict(B, g=rhs), c, Tr, dp)[:2]
    return np.concatenate([dp, dxp.reshape(-1), dxl.reshape(-1)])


def exact_residual(H, g, x):
    """g - H x without a rounding error until the last conversion (rational arithmetic over the nonzeros of H), as float64: the
    residual of a long-double solution is all cancellation, and a correction needs only its leading digits"""
    from fractions import Fraction
    fr = lambda v: Fraction(*v.as_integer_ratio())                              # noqa: E731
    xs = [fr(v) for v in x]
    r = [fr(v) for v in g]
    for i, j in zip(*np.nonzero(H)):
        r[i] -= fr(H[i, j]) * xs[j]
    return np.array([float(v) for v in r])


# ==== (c) the bound ================================================================================================================
# An entry e of a block is a sum of n_e + 1 numbers (h and a term per slot of its list), each term a double product of DL + DL
# factors.  Sequential summation of m numbers in any bracketing of depth <= m errs by at most m u sum|terms| (u = EPS / 2); a term's
# own 2 DL products and 2 DL - 2 additions by (4 DL) u |term|; h + lambda h and the last subtraction by 3 u: together less than
# EPS (n_e + 4 DL + 4) T_e with T_e the sum of absolute values, DL = 6 wherever a line can be a term.  The inverse is not exact:
# |Vinv64 - Vinv_ld| <= C_INV EPS kappa_j |Vinv_ld|, which through the same sum is C_INV EPS K_e.
def bound(n_e, DL, T_e, K_e):
    return EPS * ((np.asarray(n_e, np.float64) + 4 * DL + 4) * T_e + C_INV * K_e)


def slots_of_S(lists, nkf):
    """n_e for every entry of S: the slots of its block's pair list (the lower triangle: its mirror's)"""
    n = np.zeros((6 * nkf, 6 * nkf))
    cnt = np.diff(lists["blk_ptr"])
    blk = 0
    for k1 in range(nkf):
        for k2 in range(k1, nkf):
            n[6 * k1:6 * k1 + 6, 6 * k2:6 * k2 + 6] = cnt[blk]
            n[6 * k2:6 * k2 + 6, 6 * k1:6 * k1 + 6] = cnt[blk]
            blk += 1
    return n


def bounds_system(Tr, lists, nkf, has_lines):
    """-> (bound of S (6 nkf, 6 nkf), bound of b (6 nkf))"""
    DL = 6 if has_lines else 3
    bS = bound(slots_of_S(lists, nkf), DL, Tr["absS"], Tr["kapS"])
    bb = bound(np.repeat(np.diff(lists["kf_ptr"]), 6), DL, Tr["absb"], Tr["kapb"])
    return bS, bb


def bounds_steps(Tr, lists, absdx_pt, absdx_ls):
    """the steps: n_e = the landmark's observations + the six terms of each W dp (t itself: dp = 0, the same bound) -> (pt, ls)"""
    out = []
    for tag, DL, a, ptr in (("p", 3, absdx_pt, lists["pt_ptr"]), ("l", 6, absdx_ls, lists["ls_ptr"])):
        n = (np.diff(ptr) + 6)[:, None]
        out.append(bound(n, DL, a, Tr["kap_" + tag][:, None] * a))
    return out


def bound_sumsq(dxp, dxl, bp, bl, n_wg):
    """sum d^2: each d off by at most its bound, then a square, eight levels of the tree and the workgroups in order"""
    d = np.concatenate([np.abs(np.asarray(dxp, np.float64)).reshape(-1), np.abs(np.asarray(dxl, np.float64)).reshape(-1)])
    e = np.concatenate([bp.reshape(-1), bl.reshape(-1)])
    return float((2 * d * e + e * e).sum() + EPS * (n_wg + 10) * (d * d).sum())


def c_inv_ratio(V64, Vld, kap, singular):
    """the largest |Vinv64 - Vinv_ld|_max / (EPS kappa |Vinv_ld|_max) over the landmarks not dropped (0.0 when there is none)"""
    keep = np.flatnonzero(~singular)
    if keep.size == 0:
        return 0.0
    err = np.abs(np.asarray(V64, LD)[keep] - Vld[keep]).max(axis=(1, 2)).astype(np.float64)
    return float((err / (EPS * kap[keep] * np.abs(Vld[keep]).max(axis=(1, 2)).astype(np.float64))).max())

"""Loop-closure verification (K25 / K54, MapHandler::isLoopClosure): the records of the ABI and LcBatch (the single-pair calls are
Context's and pack their keyframes with the two helpers here), the parameter record with the shipped configuration's values, a seeded synthetic keyframe pair with known correspondences and a known relative pose, and a seeded batch of such pairs."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import synth
from ._lib import Cam, Handle, _arr, _check, _p, proto

LC_MAX_FEATURES = 16384  # include/plslam_hip.h: PLSLAM_LC_MAX_FEATURES
LC_MAX_ITERS = 10000     # include/plslam_hip.h: PLSLAM_LC_MAX_ITERS
LC_MAX_BATCH = 65536     # include/plslam_hip.h: PLSLAM_LC_MAX_BATCH


class LcParams(C.Structure):
    """plslam_lc_params (params() builds one from the shipped configuration)"""
    _fields_ = [("cam", Cam), ("homog_th", C.c_double), ("min_ratio_12_p", C.c_float), ("min_ratio_12_l", C.c_float),
                ("mutual", C.c_int32), ("has_points", C.c_int32), ("has_lines", C.c_int32), ("max_iters", C.c_int32),
                ("max_iters_ref", C.c_int32), ("reserved", C.c_int32), ("lc_inlier_ratio", C.c_double),
                ("lc_res", C.c_double), ("lc_unc", C.c_double), ("lc_inl", C.c_double), ("lc_trs", C.c_double),
                ("lc_rot", C.c_double)]


class LcKeyframe(C.Structure):
    """plslam_lc_keyframe"""
    _fields_ = [("pdesc", C.c_void_p), ("P", C.c_void_p), ("pl", C.c_void_p), ("pt_idx", C.c_void_p), ("n_pt", C.c_int32),
                ("n_ls", C.c_int32), ("ldesc", C.c_void_p), ("sPeP", C.c_void_p), ("le", C.c_void_p), ("ls_idx", C.c_void_p)]


class LcResult(C.Structure):
    """plslam_lc_result"""
    _fields_ = [(n, C.c_int32) for n in ("is_lc", "gn_ran", "common_pt", "common_ls", "n_pt_inliers", "n_ls_inliers", "iters_1",
                                          "iters_2", "ok_res", "ok_unc", "ok_inl", "ok_trs", "ok_rot", "reserved")] + \
              [(n, C.c_double) for n in ("inl_ratio_pt", "inl_ratio_ls", "e", "cov_eig", "ratio_inliers", "t", "r")] + \
              [("x_inc", C.c_double * 6), ("T_inc", C.c_double * 16), ("pose_inc", C.c_double * 6), ("H", C.c_double * 36),
               ("g", C.c_double * 6), ("clk_total", C.c_int64), ("clk_serial", C.c_int64)]

    def as_dict(self):
        """the record as plain Python values / numpy arrays (T_inc 4 x 4, H 6 x 6)"""
        d = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            d[name] = np.ctypeslib.as_array(v).copy() if not isinstance(v, (int, float)) else v
        d["T_inc"] = d["T_inc"].reshape(4, 4)
        d["H"] = d["H"].reshape(6, 6)
        return d


def _lc_kf_arrays(kf):
    """the host arrays of one keyframe dict (pdesc, P, pl, pt_idx, ldesc, sPeP, le, ls_idx), contiguous and typed"""
    out = {"pdesc": _arr(kf["pdesc"], np.uint8, (-1, 32)), "P": _arr(kf["P"], np.float64, (-1, 3)),
           "pl": _arr(kf["pl"], np.float64, (-1, 2)), "ldesc": _arr(kf["ldesc"], np.uint8, (-1, 32)),
           "sPeP": _arr(kf["sPeP"], np.float64, (-1, 6)), "le": _arr(kf["le"], np.float64, (-1, 3))}
    for k in ("pt_idx", "ls_idx"):
        out[k] = None if kf.get(k) is None else _arr(kf[k], np.int32)
    n_pt, n_ls = out["pdesc"].shape[0], out["ldesc"].shape[0]
    for k, n in (("P", n_pt), ("pl", n_pt), ("pt_idx", n_pt), ("sPeP", n_ls), ("le", n_ls), ("ls_idx", n_ls)):
        if out[k] is not None and out[k].shape[0] != n:
            raise ValueError(f"keyframe array {k} has {out[k].shape[0]} rows, its descriptors {n}")
    return out


def _lc_kf_record(a):
    # a: the arrays of _lc_kf_arrays (host) or of device tensors' addresses; the caller keeps them alive across the call
    return LcKeyframe(_p(a["pdesc"]), _p(a["P"]), _p(a["pl"]), _p(a["pt_idx"]), a["P"].shape[0], a["sPeP"].shape[0],
                      _p(a["ldesc"]), _p(a["sPeP"]), _p(a["le"]), _p(a["ls_idx"]))


_vp, _i32 = C.c_void_p, C.c_int32
proto("plslam_lc_batch_create", [_vp, C.POINTER(LcParams), _i32, C.POINTER(_vp)])
proto("plslam_lc_batch_verify", [_vp, C.POINTER(LcKeyframe), C.POINTER(LcKeyframe), _i32, C.POINTER(LcResult), _vp, _vp, _vp, _vp])
proto("plslam_lc_batch_verify_dev", [_vp, C.POINTER(LcKeyframe), C.POINTER(LcKeyframe), _i32, _vp, _vp, _vp, _vp, _vp, _vp])
proto("plslam_lc_batch_destroy", [_vp], None)


class LcBatch(Handle):
    """plslam_lc_batch: isLoopClosure for up to max_pairs candidate pairs per call (K54), with `params` fixed."""

    def __init__(self, ctx: Context, params: LcParams, max_pairs: int):
        self.params = params
        self.max_pairs = int(max_pairs)
        h = C.c_void_p()
        _check(ctx._L.plslam_lc_batch_create(ctx.handle, C.byref(params), self.max_pairs, C.byref(h)), "plslam_lc_batch_create")
        self._open(ctx, "plslam_lc_batch_destroy", h)

    def verify(self, pairs):
        """pairs: a sequence of (kf0, kf1) keyframe dicts (Context.loop_closure_verify's).  A dict that appears several
        times is packed and uploaded once.  -> one (result dict, pt_corr, pt_inlier, ls_corr, ls_inlier) per pair."""
        B = len(pairs)
        packed = {}

        def rec(kf):
            if id(kf) not in packed:
                a = _lc_kf_arrays(kf)
                packed[id(kf)] = (_lc_kf_record(a), a)
            return packed[id(kf)][0]

        r0 = (LcKeyframe * max(B, 1))(*(rec(p[0]) for p in pairs))
        r1 = (LcKeyframe * max(B, 1))(*(rec(p[1]) for p in pairs))
        rp = np.concatenate([[0], np.cumsum([r0[b].n_pt for b in range(B)])]).astype(np.int64)
        rl = np.concatenate([[0], np.cumsum([r0[b].n_ls for b in range(B)])]).astype(np.int64)
        pc, pi = np.zeros((int(rp[-1]), 4), np.int32), np.zeros(int(rp[-1]), np.uint8)
        lc, li = np.zeros((int(rl[-1]), 4), np.int32), np.zeros(int(rl[-1]), np.uint8)
        res = (LcResult * max(B, 1))()
        _check(self._L.plslam_lc_batch_verify(self._h, r0, r1, B, res, _p(pc), _p(pi), _p(lc), _p(li)), "plslam_lc_batch_verify")
        out = []
        for b in range(B):
            d = res[b].as_dict()
            n, m = d["common_pt"], d["common_ls"]
            out.append((d, pc[rp[b]:rp[b] + n], pi[rp[b]:rp[b] + n].astype(bool), lc[rl[b]:rl[b] + m],
                        li[rl[b]:rl[b] + m].astype(bool)))
        return out

    def verify_dev(self, kf0_dev, kf1_dev, results_ptr, pt_corr_ptr, pt_inlier_ptr, ls_corr_ptr, ls_inlier_ptr, stream=None):
        """Device-pointer form.  kf0_dev / kf1_dev: B dicts of device addresses each (Context.loop_closure_verify_dev's);
        results_ptr: B x sizeof(LcResult) bytes; pair b's rows start at row sum(n_pt of kf0_dev[:b]) (n_ls for lines).
        Enqueued behind `stream` (None = the context's stream), no synchronisation."""
        B = len(kf0_dev)
        if len(kf1_dev) != B:
            raise ValueError("kf0_dev and kf1_dev differ in length")

        def recs(ks):
            return (LcKeyframe * max(B, 1))(*(
                LcKeyframe(*(C.c_void_p(k.get(n) or 0) for n in ("pdesc", "P", "pl", "pt_idx")), int(k["n_pt"]), int(k["n_ls"]),
                           *(C.c_void_p(k.get(n) or 0) for n in ("ldesc", "sPeP", "le", "ls_idx"))) for k in ks))

        _check(self._L.plslam_lc_batch_verify_dev(self._h, recs(kf0_dev), recs(kf1_dev), B, C.c_void_p(results_ptr or 0),
                                                  C.c_void_p(pt_corr_ptr or 0), C.c_void_p(pt_inlier_ptr or 0),
                                                  C.c_void_p(ls_corr_ptr or 0), C.c_void_p(ls_inlier_ptr or 0),
                                                  C.c_void_p(stream or 0)), "plslam_lc_batch_verify_dev")


# config/config/config.yaml (SlamConfig) and the stvo-pl Config it loads (homog_th, min_ratio_12_*, best_lr_matches)
DEFAULTS = dict(homog_th=1e-7, min_ratio_12_p=0.75, min_ratio_12_l=0.75, mutual=1, has_points=1, has_lines=1, max_iters=5,
                max_iters_ref=10, lc_inlier_ratio=30.0, lc_res=1.5, lc_unc=0.01, lc_inl=0.3, lc_trs=1.5, lc_rot=35.0)
KITTI_ITERS = dict(max_iters=100, max_iters_ref=100)     # config/config/config_kitti.yaml:49-50


def params(cam=None, **over) -> LcParams:
    """plslam_lc_params with DEFAULTS, overridden by keyword; cam: a Cam, or a dict of fx, fy, cx, cy (default EuRoC)"""
    d = dict(DEFAULTS)
    unknown = set(over) - set(d)
    if unknown:
        raise KeyError(f"unknown loop-closure parameters: {sorted(unknown)}")
    d.update(over)
    if cam is None:
        cam = synth.EUROC
    if not isinstance(cam, Cam):
        cam = Cam(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam.get("b", 0.0), cam.get("width", 0), cam.get("height", 0))
    p = LcParams()
    p.cam = cam
    for k, v in d.items():
        setattr(p, k, v)
    return p


def params_dict(p: LcParams) -> dict:
    return {k: getattr(p, k) for k in DEFAULTS}


def _project(cam, X):
    return np.stack([cam["cx"] + cam["fx"] * X[:, 0] / X[:, 2], cam["cy"] + cam["fy"] * X[:, 1] / X[:, 2]], axis=1)


def _disk(rng, n, radius):
    a = rng.uniform(0, 2 * np.pi, n)
    r = radius * np.sqrt(rng.uniform(0, 1, n))
    return np.stack([r * np.cos(a), r * np.sin(a)], axis=1)


def keyframe_pair(seed, n_pt=1500, n_ls=200, pose=(0.05, -0.03, 0.10, 0.01, -0.02, 0.015), keep_frac=0.7, flip_p=0.08,
                  outlier_frac=0.1, noise_px=0.5, outlier_px=(12.0, 40.0), cam=None):
    """Two keyframes whose features partly observe the same scene.  kf0 holds n_pt points (P in kf0's frame, 2-20 m deep)
    and n_ls segments; kf1's descriptors are synth.noisy_copy of kf0's (keep_frac true rows with flip_p bit flips, the
    rest fresh distractors), and a true row's observation is the projection of T * X (T = expmap(pose), kf0 -> kf1) with
    noise inside a disk of noise_px.  outlier_frac of the true rows are moved by outlier_px (a range) instead.  A point
    observation is pl; a line's is le, the normalised line through its projected end points.  Returns (kf0, kf1, truth)."""
    cam = cam or synth.EUROC
    rng = np.random.Generator(np.random.PCG64(seed))
    T = synth.se3_exp(np.asarray(pose, np.float64))
    W, Hh = cam.get("width", 752), cam.get("height", 480)

    def scene(n):
        uv = np.stack([rng.uniform(40, W - 40, n), rng.uniform(40, Hh - 40, n)], axis=1)
        z = rng.uniform(2.0, 20.0, n)
        return np.stack([(uv[:, 0] - cam["cx"]) * z / cam["fx"], (uv[:, 1] - cam["cy"]) * z / cam["fy"], z], axis=1)

    def xf(X):
        return X @ T[:3, :3].T + T[:3, 3]

    kf0, kf1, truth = {}, {}, {"T": T, "pose": np.asarray(pose, np.float64)}
    # points
    P = scene(n_pt)
    d0 = synth.random_desc(rng, n_pt)
    if n_pt:
        d1, perm, fresh = synth.noisy_copy(rng, d0, keep_frac, flip_p)
    else:
        d1, perm, fresh = d0.copy(), np.zeros(0, np.int64), np.zeros(0, bool)
    pl = _project(cam, xf(P[perm])) + _disk(rng, n_pt, noise_px) if n_pt else np.zeros((0, 2))
    out = (~fresh) & (rng.random(n_pt) < outlier_frac)
    if out.any():
        pl[out] += _ring(rng, int(out.sum()), *outlier_px)
    pl[fresh] = np.stack([rng.uniform(0, W, int(fresh.sum())), rng.uniform(0, Hh, int(fresh.sum()))], axis=1)
    kf0.update(pdesc=d0, P=P, pt_idx=np.arange(n_pt, dtype=np.int32) + 1000)
    kf1.update(pdesc=d1, pl=pl, pt_idx=np.arange(n_pt, dtype=np.int32) + 5000)
    truth.update(pt_src=np.where(fresh, -1, perm), pt_out=out)
    kf0["pl"] = _project(cam, P)
    kf1["P"] = xf(P[perm]) if n_pt else np.zeros((0, 3))
    # lines
    S, E = scene(n_ls), scene(n_ls)
    l0 = synth.random_desc(rng, n_ls)
    if n_ls:
        l1, lperm, lfresh = synth.noisy_copy(rng, l0, keep_frac, flip_p)
    else:
        l1, lperm, lfresh = l0.copy(), np.zeros(0, np.int64), np.zeros(0, bool)
    s1 = _project(cam, xf(S[lperm])) + _disk(rng, n_ls, noise_px) if n_ls else np.zeros((0, 2))
    e1 = _project(cam, xf(E[lperm])) + _disk(rng, n_ls, noise_px) if n_ls else np.zeros((0, 2))
    lout = (~lfresh) & (rng.random(n_ls) < outlier_frac)
    if lout.any():                     # moved across the segment: a shift along it would leave the line in place
        dvec = e1[lout] - s1[lout]
        nrm = np.stack([-dvec[:, 1], dvec[:, 0]], axis=1) / np.linalg.norm(dvec, axis=1)[:, None]
        sh = nrm * (rng.uniform(*outlier_px, int(lout.sum())) * rng.choice([-1.0, 1.0], int(lout.sum())))[:, None]
        s1[lout] += sh
        e1[lout] += sh
    nf = int(lfresh.sum())
    s1[lfresh] = np.stack([rng.uniform(0, W, nf), rng.uniform(0, Hh, nf)], axis=1)
    e1[lfresh] = np.stack([rng.uniform(0, W, nf), rng.uniform(0, Hh, nf)], axis=1)
    le = np.cross(np.c_[s1, np.ones(n_ls)], np.c_[e1, np.ones(n_ls)]) if n_ls else np.zeros((0, 3))
    if n_ls:
        le = le / np.sqrt(le[:, 0] ** 2 + le[:, 1] ** 2)[:, None]
    kf0.update(ldesc=l0, sPeP=np.c_[S, E], ls_idx=np.arange(n_ls, dtype=np.int32) + 2000)
    kf1.update(ldesc=l1, le=le, ls_idx=np.arange(n_ls, dtype=np.int32) + 7000)
    kf0["le"] = np.zeros((n_ls, 3))
    kf1["sPeP"] = np.c_[xf(S[lperm]), xf(E[lperm])] if n_ls else np.zeros((0, 6))
    truth.update(ls_src=np.where(lfresh, -1, lperm), ls_out=lout)
    for kf in (kf0, kf1):
        for k, w in (("pdesc", 32), ("P", 3), ("pl", 2), ("ldesc", 32), ("sPeP", 6), ("le", 3)):
            kf[k] = np.ascontiguousarray(np.asarray(kf[k]).reshape(-1, w), dtype=np.uint8 if "desc" in k else np.float64)
    return kf0, kf1, truth


# what keyframe_batch cycles through: the sizes of the library's three workloads, and per pair one of these changes to
# keyframe_pair's defaults -- a plain pair, too few true rows for the inlier-ratio gate, a translation beyond lcTrs, a roll
# beyond lcRot, a keyframe pair without lines, one without points, and two more plain pairs at other poses
BATCH_SIZES = ((1500, 200), (800, 100), (4000, 600))
BATCH_VARIANTS = (
    dict(),
    dict(keep_frac=0.2),
    dict(pose=(1.3, -0.9, 0.8, 0.01, -0.02, 0.015)),
    dict(pose=(0.05, -0.03, 0.10, 0.0, 0.0, 0.63)),
    dict(n_ls=0),
    dict(n_pt=0),
    dict(pose=(-0.2, 0.1, 0.3, -0.03, 0.02, 0.05)),
    dict(pose=(0.4, 0.2, -0.1, 0.02, 0.04, -0.06), keep_frac=0.5),
)


def keyframe_batch(seed, B, sizes=BATCH_SIZES, variants=BATCH_VARIANTS, **kw):
    """B keyframe pairs for one batched call: pair b is keyframe_pair(1000 * seed + b, *sizes[b % len(sizes)]) with
    variants[b % len(variants)] (and kw) over its defaults.  Deterministic in (seed, B, sizes, variants, kw); pair b does not
    depend on B.  Returns a list of (kf0, kf1, truth)."""
    out = []
    for b in range(B):
        n_pt, n_ls = sizes[b % len(sizes)]
        a = dict(n_pt=n_pt, n_ls=n_ls)
        a.update(kw)
        a.update(variants[b % len(variants)])
        out.append(keyframe_pair(1000 * int(seed) + b, **a))
    return out


def _ring(rng, n, r0, r1):
    a = rng.uniform(0, 2 * np.pi, n)
    r = rng.uniform(r0, r1, n)
    return np.stack([r * np.cos(a), r * np.sin(a)], axis=1)

"""Tracking a batch of stereo pairs on the device (include/plslam_track.h; K108-K110 in front of K54): the records of that
header, TrackBatch, the one-frame back-projection, and a seeded synthetic batch of stereo pairs with a known motion each."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import synth
from ._lib import Cam, Handle, _check, _p, proto_in
from .loop_closure import LcParams, LcResult, _ring

HEADER = "plslam_track.h"


class TrackPair(C.Structure):
    """plslam_track_pair (device pointers)"""
    _fields_ = [("m_pt", C.c_void_p), ("st_pt_prev", C.c_void_p), ("disp_pt_prev", C.c_void_p), ("kp_prev", C.c_void_p),
                ("st_pt_curr", C.c_void_p), ("kp_curr", C.c_void_p), ("n_pt_prev", C.c_int32), ("n_pt_curr", C.c_int32),
                ("m_ls", C.c_void_p), ("st_ls_prev", C.c_void_p), ("disp_ls_prev", C.c_void_p), ("seg_prev", C.c_void_p),
                ("st_ls_curr", C.c_void_p), ("seg_curr", C.c_void_p), ("n_ls_prev", C.c_int32), ("n_ls_curr", C.c_int32)]


class TrackBuffers(C.Structure):
    """plslam_track_buffers"""
    _fields_ = [(n, C.c_void_p) for n in ("pt_off", "ls_off", "pt_rows", "ls_rows", "P", "pl_obs", "sPeP", "le_obs", "pt_inlier",
                                           "ls_inlier", "results")] + \
               [("pt_capacity", C.c_int64), ("ls_capacity", C.c_int64), ("B", C.c_int32), ("reserved", C.c_int32)]


_vp, _i32 = C.c_void_p, C.c_int32
proto_in(HEADER, "plslam_track_batch_create", [_vp, C.POINTER(LcParams), C.POINTER(TrackPair), _i32, C.POINTER(_vp)])
proto_in(HEADER, "plslam_track_batch_run", [_vp, _vp])
proto_in(HEADER, "plslam_track_batch_device_buffers", [_vp, C.POINTER(TrackBuffers)])
proto_in(HEADER, "plslam_track_batch_download", [_vp] * 12)
proto_in(HEADER, "plslam_track_batch_destroy", [_vp], None)
proto_in(HEADER, "plslam_stereo_backproject_dev", [_vp, C.POINTER(Cam), _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp])

_PAIR_POINTERS = tuple(n for n, t in TrackPair._fields_ if t is C.c_void_p)
_PAIR_COUNTS = tuple(n for n, t in TrackPair._fields_ if t is C.c_int32)


def track_pair(**kw) -> TrackPair:
    """A plslam_track_pair from device addresses (ints; 0 / None / absent: NULL) and the four counts (absent: 0)."""
    unknown = set(kw) - set(_PAIR_POINTERS) - set(_PAIR_COUNTS)
    if unknown:
        raise KeyError(f"unknown fields of plslam_track_pair: {sorted(unknown)}")
    p = TrackPair()
    for n in _PAIR_POINTERS:
        setattr(p, n, kw.get(n) or None)
    for n in _PAIR_COUNTS:
        setattr(p, n, int(kw.get(n, 0)))
    return p


class TrackBatch(Handle):
    """plslam_track_batch: B stereo pairs over device pointers, created once; every run() turns the tables they name into packed
    correspondences and the relative pose of every pair, enqueued on a stream.  pairs: TrackPair records or dicts of their
    fields (track_pair)."""

    def __init__(self, ctx: "Context", params: LcParams, pairs):
        pairs = [p if isinstance(p, TrackPair) else track_pair(**p) for p in pairs]
        self.params, self.B = params, len(pairs)
        arr = (TrackPair * max(self.B, 1))(*pairs)
        h = C.c_void_p()
        _check(ctx._L.plslam_track_batch_create(ctx.handle, C.byref(params), arr, self.B, C.byref(h)), "plslam_track_batch_create")
        self._open(ctx, "plslam_track_batch_destroy", h)

    def run(self, stream: int = 0) -> None:
        """Enqueue only: K108, K109, K110 and K54 behind `stream` (0 = the context's stream)."""
        _check(self._L.plslam_track_batch_run(self._h, stream or None), "plslam_track_batch_run")

    def device_buffers(self) -> TrackBuffers:
        b = TrackBuffers()
        _check(self._L.plslam_track_batch_device_buffers(self._h, C.byref(b)), "plslam_track_batch_device_buffers")
        return b

    def download(self) -> dict:
        """Every output as a host array, after a synchronisation (tests and tools): pt_off, ls_off, the row arrays IN FULL (to their
        capacity; pair b's rows are [off[b], off[b + 1])), the masks, and `results`, a list of B result dicts."""
        b = self.device_buffers()
        np_, nl, B = int(b.pt_capacity), int(b.ls_capacity), self.B
        o = {"pt_off": np.zeros(B + 1, np.int32), "ls_off": np.zeros(B + 1, np.int32),
             "pt_rows": np.zeros((np_, 2), np.int32), "ls_rows": np.zeros((nl, 2), np.int32),
             "P": np.zeros((np_, 3)), "pl_obs": np.zeros((np_, 2)), "sPeP": np.zeros((nl, 6)), "le_obs": np.zeros((nl, 3)),
             "pt_inlier": np.zeros(np_, np.uint8), "ls_inlier": np.zeros(nl, np.uint8)}
        res = (LcResult * max(B, 1))()
        _check(self._L.plslam_track_batch_download(self._h, *(_p(o[k]) if o[k].size else None for k in o), C.addressof(res)),
               "plslam_track_batch_download")
        o["results"] = [res[i].as_dict() for i in range(B)]
        return o


def backproject_dev(ctx, cam: Cam, stereo_12: int, disp: int, f_l: int, n_l: int, lines: bool, out_a: int, out_b: int,
                    stream: int = 0) -> None:
    """plslam_stereo_backproject_dev: one frame's P / pl (points) or sPeP / le (lines) by left row, device addresses."""
    _check(ctx._L.plslam_stereo_backproject_dev(ctx.handle, C.byref(cam), stereo_12 or None, disp or None, f_l or None, int(n_l),
                                                int(bool(lines)), out_a or None, out_b or None, stream or None),
           "plslam_stereo_backproject_dev")


# ---- a seeded batch of stereo pairs ------------------------------------------------------------------------------------------
# A rectified stereo camera: backProjection scales both image axes by b / d = z / fx, so it inverts the projection only where
# fy = fx (EuRoC's raw intrinsics differ by 0.3 %, which would bias every recovered motion)
SCENE_CAM = synth.KITTI00

def _project(cam, X):
    return np.stack([cam["cx"] + cam["fx"] * X[:, 0] / X[:, 2], cam["cy"] + cam["fy"] * X[:, 1] / X[:, 2]], axis=1)


def _right(cam, uv, z):
    """kp_r = kp_l - (fx * b / z, 0)"""
    return uv - np.stack([cam["fx"] * cam["b"] / z, np.zeros_like(z)], axis=1)


def _disk(rng, n, radius):
    a = rng.uniform(0, 2 * np.pi, n)
    r = radius * np.sqrt(rng.uniform(0, 1, n))
    return np.stack([r * np.cos(a), r * np.sin(a)], axis=1)


def _anywhere(rng, n, W, Hh):
    return np.stack([rng.uniform(0, W, n), rng.uniform(0, Hh, n)], axis=1)


def _inverse_perm(perm, fresh, n):
    """table[i] = the row k with perm[k] == i that is not fresh, or -1"""
    t = np.full(n, -1, np.int32)
    k = np.flatnonzero(~fresh)
    t[perm[k]] = k
    return t


def _copy(rng, d, keep_frac, flip_p):
    if d.shape[0] == 0:
        return d.copy(), np.zeros(0, np.int64), np.zeros(0, bool)
    return synth.noisy_copy(rng, d, keep_frac, flip_p)


def track_pair_scene(seed, n_pt=300, n_ls=60, pose=(0.05, -0.03, 0.10, 0.01, -0.02, 0.015), keep_frac=0.7, stereo_frac=0.8,
                     flip_p=0.08, outlier_frac=0.1, noise_px=0.5, outlier_px=(12.0, 40.0), cam=None):
    """One stereo pair (prev, curr).  prev-L holds n_pt points (3-30 m deep in prev's frame) and n_ls segments whose end points
    are about equally deep; T = expmap(pose) takes prev's frame to curr's.  Every other image is a synth.noisy_copy of a left
    one: prev-R of prev-L and curr-R of curr-L (stereo_frac of the rows true, the others fresh: their left rows are non-stereo),
    curr-L of prev-L (keep_frac true rows, the rest fresh features at depths of their own).  A true right feature sits at
    kp_l - (fx b / z, 0); a true curr-L feature at the projection of T X with noise inside a disk of noise_px, outlier_frac of
    them moved by outlier_px instead (segments across themselves).  Key points and segments are float32.
    Returns a dict: desc / kp per image (pdesc_pl, kp_pl, ... ldesc_cr, seg_cr with pl, pr, cl, cr = prev-L, prev-R, curr-L,
    curr-R), the true tables m_pt, st_pt_prev, st_pt_curr, m_ls, st_ls_prev, st_ls_curr (row of the other image or -1), the
    outlier flags by curr-L row, X / S / E, T and pose."""
    cam = cam or SCENE_CAM
    rng = np.random.Generator(np.random.PCG64(seed))
    T = synth.se3_exp(np.asarray(pose, np.float64))
    W, Hh = cam.get("width", 1241), cam.get("height", 376)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)      # noqa: E731

    def back(uv, z):
        return np.stack([(uv[:, 0] - cam["cx"]) * z / cam["fx"], (uv[:, 1] - cam["cy"]) * z / cam["fy"], z], axis=1)

    def xf(X):
        return X @ T[:3, :3].T + T[:3, 3]

    out = {"T": T, "pose": np.asarray(pose, np.float64), "cam": dict(cam)}
    # ---- points
    X = back(np.stack([rng.uniform(40, W - 40, n_pt), rng.uniform(40, Hh - 40, n_pt)], axis=1), rng.uniform(3.0, 30.0, n_pt))
    d_pl = synth.random_desc(rng, n_pt)
    d_pr, rperm, rfresh = _copy(rng, d_pl, stereo_frac, flip_p)
    kp_pl = _project(cam, X)
    kp_pr = _right(cam, kp_pl[rperm], X[rperm, 2])
    kp_pr[rfresh] = _anywhere(rng, n_pt, W, Hh)[rfresh]
    d_cl, cperm, cfresh = _copy(rng, d_pl, keep_frac, flip_p)
    Xc = xf(X[cperm])
    Xc[cfresh] = back(_anywhere(rng, n_pt, W, Hh), rng.uniform(3.0, 30.0, n_pt))[cfresh]
    kp_cl = _project(cam, Xc)
    moved = (~cfresh) & (rng.random(n_pt) < outlier_frac)
    shift = _disk(rng, n_pt, noise_px)
    kp_cl = kp_cl + np.where(moved[:, None], _ring(rng, n_pt, *outlier_px), np.where(cfresh[:, None], 0.0, shift))
    d_cr, crperm, crfresh = _copy(rng, d_cl, stereo_frac, flip_p)
    kp_cr = _right(cam, kp_cl[crperm], Xc[crperm, 2])
    kp_cr[crfresh] = _anywhere(rng, n_pt, W, Hh)[crfresh]
    out.update(pdesc_pl=d_pl, pdesc_pr=d_pr, pdesc_cl=d_cl, pdesc_cr=d_cr, kp_pl=f32(kp_pl), kp_pr=f32(kp_pr), kp_cl=f32(kp_cl),
               kp_cr=f32(kp_cr), X=X, m_pt=_inverse_perm(cperm, cfresh, n_pt), st_pt_prev=_inverse_perm(rperm, rfresh, n_pt),
               st_pt_curr=_inverse_perm(crperm, crfresh, n_pt), pt_out=moved)
    # ---- segments: E at 30-120 px from S, at least 0.2 rad off the horizontal, 0.9-1.1 times as deep
    s_uv = np.stack([rng.uniform(60, W - 60, n_ls), rng.uniform(60, Hh - 60, n_ls)], axis=1)
    ang = rng.uniform(0.2, np.pi - 0.2, n_ls) * rng.choice([-1.0, 1.0], n_ls)
    e_uv = s_uv + rng.uniform(30, 120, n_ls)[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    zs = rng.uniform(3.0, 30.0, n_ls)
    S, E = back(s_uv, zs), back(e_uv, zs * rng.uniform(0.9, 1.1, n_ls))
    l_pl = synth.random_desc(rng, n_ls)
    l_pr, rperm, rfresh = _copy(rng, l_pl, stereo_frac, flip_p)
    seg_pl = np.c_[_project(cam, S), _project(cam, E)]
    seg_pr = np.c_[_right(cam, seg_pl[rperm, :2], S[rperm, 2]), _right(cam, seg_pl[rperm, 2:], E[rperm, 2])]
    seg_pr[rfresh] = np.c_[_anywhere(rng, n_ls, W, Hh), _anywhere(rng, n_ls, W, Hh)][rfresh]
    l_cl, cperm, cfresh = _copy(rng, l_pl, keep_frac, flip_p)
    Sc, Ec = xf(S[cperm]), xf(E[cperm])
    fs = _anywhere(rng, n_ls, W, Hh)
    fz = rng.uniform(3.0, 30.0, n_ls)
    Sc[cfresh] = back(fs, fz)[cfresh]
    Ec[cfresh] = back(fs + rng.uniform(30, 120, n_ls)[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1), fz)[cfresh]
    s1, e1 = _project(cam, Sc), _project(cam, Ec)
    lmoved = (~cfresh) & (rng.random(n_ls) < outlier_frac)
    ns, ne = _disk(rng, n_ls, noise_px), _disk(rng, n_ls, noise_px)
    dvec = e1 - s1
    across = np.stack([-dvec[:, 1], dvec[:, 0]], axis=1) / np.maximum(np.linalg.norm(dvec, axis=1), 1e-9)[:, None]
    across = across * (rng.uniform(*outlier_px, n_ls) * rng.choice([-1.0, 1.0], n_ls))[:, None]
    s1 = s1 + np.where(lmoved[:, None], across, np.where(cfresh[:, None], 0.0, ns))
    e1 = e1 + np.where(lmoved[:, None], across, np.where(cfresh[:, None], 0.0, ne))
    seg_cl = np.c_[s1, e1]
    l_cr, crperm, crfresh = _copy(rng, l_cl, stereo_frac, flip_p)
    seg_cr = np.c_[_right(cam, seg_cl[crperm, :2], Sc[crperm, 2]), _right(cam, seg_cl[crperm, 2:], Ec[crperm, 2])]
    seg_cr[crfresh] = np.c_[_anywhere(rng, n_ls, W, Hh), _anywhere(rng, n_ls, W, Hh)][crfresh]
    out.update(ldesc_pl=l_pl, ldesc_pr=l_pr, ldesc_cl=l_cl, ldesc_cr=l_cr, seg_pl=f32(seg_pl).reshape(-1, 4),
               seg_pr=f32(seg_pr).reshape(-1, 4), seg_cl=f32(seg_cl).reshape(-1, 4), seg_cr=f32(seg_cr).reshape(-1, 4), S=S, E=E,
               m_ls=_inverse_perm(cperm, cfresh, n_ls), st_ls_prev=_inverse_perm(rperm, rfresh, n_ls),
               st_ls_curr=_inverse_perm(crperm, crfresh, n_ls), ls_out=lmoved)
    return out


# the motions track_scene cycles through, pair by pair
SCENE_POSES = ((0.05, -0.03, 0.10, 0.01, -0.02, 0.015), (-0.08, 0.02, 0.15, -0.015, 0.01, 0.02), (0.02, 0.04, 0.25, 0.0, 0.03, -0.01),
               (0.0, 0.0, 0.05, 0.02, 0.0, 0.0))


def track_scene(seed, B, n_pt=300, n_ls=60, sizes=None, **kw):
    """B stereo pairs: pair b is track_pair_scene(1000 * seed + b) at SCENE_POSES[b % 4] with n_pt / n_ls features, or
    sizes[b] = (n_pt, n_ls) where given (a pair without lines, one without points).  Pair b does not depend on B."""
    out = []
    for b in range(B):
        npt, nls = sizes[b] if sizes is not None else (n_pt, n_ls)
        a = dict(pose=SCENE_POSES[b % len(SCENE_POSES)])
        a.update(kw)
        out.append(track_pair_scene(1000 * int(seed) + b, npt, nls, **a))
    return out


def true_disparities(pair, which="p"):
    """The disparities of the TRUE stereo tables of one image pair of a scene pair (which: "p" prev, "c" curr), as the stereo
    gates form them: points n doubles, the float32 difference x_l - x_r widened; lines n x 2 (start, end: the right end points
    lie on the left ones' rows already, so the gate's slide along the right line moves them by rounding only); 0 where the left
    row is not stereo."""
    st, kl, kr = pair[f"st_pt_{'prev' if which == 'p' else 'curr'}"], pair[f"kp_{which}l"], pair[f"kp_{which}r"]
    dp = np.where(st >= 0, (kl[:, 0] - kr[np.maximum(st, 0), 0]).astype(np.float64), 0.0) if st.size else np.zeros(0)
    sl, gl, gr = pair[f"st_ls_{'prev' if which == 'p' else 'curr'}"], pair[f"seg_{which}l"].astype(np.float64), pair[f"seg_{which}r"].astype(np.float64)
    if sl.size:
        j = np.maximum(sl, 0)
        dl = np.where((sl >= 0)[:, None], np.stack([gl[:, 0] - gr[j, 0], gl[:, 2] - gr[j, 2]], axis=1), 0.0)
    else:
        dl = np.zeros((0, 2))
    return dp, dl

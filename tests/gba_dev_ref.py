"""A literal, sequential restatement of the gather of MapHandler::globalBundleAdjustment (src/mapHandler.cpp:1995-2092) over the
CSR image of the map (plslam_amd.local_map.synthetic_map, plslam_amd.gba.map_image): what plslam_local_map_form_all +
plslam_local_map_gather compute on the device.  The line numbers cited are the reference's.  numpy only.

Also the expected outputs the device tests of the resident route share: the host builder's lists come from the library itself
(a host-built plan), so nothing else is restated here."""
from __future__ import annotations

import numpy as np


def gba_gather(m):
    """-> dict(kf_list, pt_list, ls_list, pt_obs (n, 6), ls_obs (n, 6), pt_obs_uv, ls_l_obs, X_aux), order for order"""
    X_aux, kf_list = [], []
    for k in range(m["n_map_kf"]):                                    # :2002
        if m["kf_valid"][k] and k != 0:                               # :2004 `!= NULL`, :2006 `kf_idx != 0`
            X_aux.extend(m["x_kf_w"][k].tolist())                     # :2008-2010
            kf_list.append(k)                                         # :2011
    out = {}
    for kind, tag in (("points", "pt"), ("lines", "ls")):
        A = m[kind]
        valid, obs_ptr, obs_kf = A["valid"].tolist(), A["obs_ptr"].tolist(), A["obs_kf"].tolist()
        obs, src, lst = [], [], []
        lm_local_idx = 0                                              # :2019 / :2057
        for i in range(A["n"]):                                       # :2020 / :2058
            if not valid[i]:                                          # :2022 / :2060
                continue
            # (:2024-2026 / :2062-2064: X_aux takes the landmark here; the rows are copied behind the loop, in this order)
            for o in range(obs_ptr[i + 1] - obs_ptr[i]):              # :2028 / :2066
                kf = obs_kf[obs_ptr[i] + o]                           # :2034
                loc = -1                                              # :2036
                for j, kj in enumerate(kf_list):                      # :2038-2045: the linear search
                    if kj == kf:
                        loc = j
                        break
                obs.append((i, lm_local_idx, o, kf, loc, 1))          # :2031-2037, :2046
                src.append(obs_ptr[i] + o)
            lm_local_idx += 1                                         # :2048
            lst.append(i)                                             # :2050
        X_aux.extend(A["X"][lst].ravel().tolist())
        out[tag + "_list"] = np.array(lst, np.int32)
        out[tag + "_obs"] = np.array(obs, np.int32).reshape(-1, 6)
        out["pt_obs_uv" if tag == "pt" else "ls_l_obs"] = A["obs_val"][src].reshape(-1, A["obs_val"].shape[1])
    out["kf_list"] = np.array(kf_list, np.int32)
    out["X_aux"] = np.array(X_aux, np.float64)
    return out


GATHER_KEYS = ("kf_list", "pt_list", "ls_list", "pt_obs", "ls_obs", "pt_obs_uv", "ls_l_obs", "X_aux")


def same_bits(a, b):
    """equal as bit patterns (NaN equals the same NaN), same shape and type"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()

"""The batch the K54 tests run (tests/test_lc_batch_cpu.py pins what it covers; tests/test_gpu_lc_batch.py runs it on the
device): eight seeded pairs of plslam_amd.loop_closure.keyframe_batch under five parameter sets."""
import numpy as np

from plslam_amd import loop_closure as LC, synth
from oracle import oracle as O

import lc_ref

SEED, B = 7, 8
# the three feature modes of the source, and two sets whose threshold sits under what every pair of the batch reaches: the
# residual test and the uncertainty test then reject the pairs the other tests accept (translation and rotation are rejected
# by the data: pairs 2 and 3 of the batch)
PARAM_SETS = {"pl": dict(), "p": dict(has_lines=0), "l": dict(has_points=0), "res": dict(lc_res=0.05), "unc": dict(lc_unc=1e-6)}
OCAM = O.make_cam(**synth.EUROC)
_pairs = {}
_refs = {}


def pairs(seed=SEED, n=B, **kw):
    key = (seed, n, tuple(sorted(kw.items())))
    if key not in _pairs:
        _pairs[key] = LC.keyframe_batch(seed, n, **kw)
    return _pairs[key]


def reference(name, b):
    """lc_ref.is_loop_closure of pair b of the test batch under PARAM_SETS[name] -> (ref, params dict)"""
    prm = LC.params_dict(LC.params(**PARAM_SETS[name]))
    if (name, b) not in _refs:
        kf0, kf1, _ = pairs()[b]
        _refs[(name, b)] = lc_ref.is_loop_closure(prm, OCAM, kf0, kf1)
    return _refs[(name, b)], prm


def same_result(a, b):
    """two plslam_lc_result dicts agree in every bit of every field but the two clocks"""
    for k, v in a.items():
        if k in ("clk_total", "clk_serial"):
            continue
        x, y = np.asarray(v), np.asarray(b[k])
        if x.dtype.kind == "f":
            if not np.array_equal(x.view(np.uint64) if x.ndim else np.float64(x).view(np.uint64),
                                  y.view(np.uint64) if y.ndim else np.float64(y).view(np.uint64)):
                return False
        elif not np.array_equal(x, y):
            return False
    return True

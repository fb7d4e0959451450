"""bench.py's input generator (make_inputs): the batches it builds in pieces, in worker processes, are bit for bit what
synth.stereo_stream / synth.stereo_geometry return for the whole batch -- at shard starts on and off the frame chain's
64-frame restarts, with and without the gate stage's geometry.  No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from plslam_amd import synth  # noqa: E402


@pytest.mark.parametrize("B,first_pair,workers", [(150, 0, 3), (70, 37, 2), (130, 64, 4), (129, 65, 1), (5, 200, 3)])
def test_make_inputs_equals_synth(B, first_pair, workers):
    n_orb, n_lbd = 48, 12
    seeds = [synth.SEED0, synth.SEED0 + 7919]
    got = bench.make_inputs(B, n_orb, n_lbd, first_pair, seeds, True, workers)
    assert len(got) == len(seeds)
    for seed, (st, geo) in zip(seeds, got):
        ref = synth.stereo_stream(B, n_orb, n_lbd, seed=seed, first_pair=first_pair)
        ref_geo = synth.stereo_geometry(ref, first_pair=first_pair)
        assert sorted(st) == sorted(ref) and sorted(geo) == sorted(ref_geo)
        for k, v in ref.items():
            assert st[k].dtype == v.dtype and st[k].shape == v.shape and np.array_equal(st[k], v), k
        for k, v in ref_geo.items():
            assert geo[k].dtype == v.dtype and np.array_equal(geo[k].view(np.uint32), v.view(np.uint32)), k


def test_make_inputs_without_geometry():
    st, geo = bench.make_inputs(80, 32, 8, 0, [synth.SEED0 + 3], False, 2)[0]
    ref = synth.stereo_stream(80, 32, 8, seed=synth.SEED0 + 3, first_pair=0)
    assert geo is None and all(np.array_equal(st[k], v) for k, v in ref.items())

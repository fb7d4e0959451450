"""ctypes binding of include/plslam_hip.h (libplslam_hip.so): the names of every concern module under one roof.

The binding itself lives one module per concern -- _lib (loading, prototypes, the handle life cycle), context, match, lba, gba,
pgo, bow, loop_closure, and local_map / map_insert / lc_fuse / map_lists for the device-resident map -- each with its structs,
its prototypes and its wrappers together.  This module only imports them.  There is NO CPU fallback.
"""
from __future__ import annotations  # noqa: F401

import ctypes as C  # noqa: F401
import os  # noqa: F401

import numpy as np  # noqa: F401

from . import _lib, lc_fuse, local_map, map_insert, map_lists, track  # noqa: F401 (the last five: their prototypes; track's are include/plslam_track.h's, in _lib.HEADER_PROTOTYPES)
from ._lib import (ABI_VERSION, EHIP, EINVAL, ENODEV, ENOMEM, ENOTSUP, ERANGE, LIB_PATH, OK, PROTOTYPES, Handle,  # noqa: F401
                   PlslamError, _HERE, _addressof, _arr, _check, _from_buffer, _hip_memcpy_dtod, _p,
                   _preload_shared_hip_runtime, load, proto)
from .bow import (BOW_BINARY, BOW_IDF, BOW_L1_NORM, BOW_MAX_SET, BOW_NODE_DTYPE, BOW_TF, BOW_TF_IDF, BOW_WORD_DTYPE,  # noqa: F401
                  BowDatabase, BowPlStats, BowVocabDesc, BowVocabulary, _bow_stats)
from .context import (LBD_LINE_DTYPE, SCAN_AUTO, SCAN_LANE_PER_QUERY, SCAN_MFMA, SCAN_SYMMETRIC, SCAN_WAVE_PER_QUERY,  # noqa: F401
                      Cam, Context, FastMatching, PinnedArray, _fast_matching, make_cam)
from .gba import (GBA_LIST_NAMES, GBA_MAX_KEYFRAMES, GBA_STOP_DX, GBA_STOP_ERR, GBA_STOP_MAX_ITERS, GbaListSizes, GbaLists,  # noqa: F401
                  GbaPlan, GbaResult, GbaSolve, dense_ldlt_solve)
from .lba import (LBA_SOLVE_MAX_N6, LBA_STOP_DX, LBA_STOP_ERR, LBA_STOP_MAX_ITERS, LBA_STOP_NOT_PD, LbaLmParams, LbaPlan,  # noqa: F401
                  LbaResult, LbaSolve)
from .loop_closure import (LC_MAX_BATCH, LC_MAX_FEATURES, LC_MAX_ITERS, LcBatch, LcKeyframe, LcParams, LcResult,  # noqa: F401
                           _lc_kf_arrays, _lc_kf_record)
from .match import (MAX_TRAIN_ROWS, ArenaProblem, GatherStep, GridPlan, GridProblem, MatchPipeline, MatchPlan, MatchProblem,  # noqa: F401
                    PlanInfo, StereoGateProblem, grid_pair_capacity)
from .pgo import (PGO_STOP_MAX_ITERS, PGO_STOP_TERMINATE, LcImageCounts, LcImageDst, LcLandmarks, PgoParams, PgoPlan,  # noqa: F401
                  PgoResult, PgoTrial, _landmarks, correct_map, correct_map_dev, envelope_ldlt_solve)

# every symbol include/plslam_hip.h declares (tests check the .so exports all of them): taken here, after every concern module
# has stated its prototypes
ABI_SYMBOLS = tuple(PROTOTYPES)

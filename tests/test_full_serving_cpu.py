"""Serving full-covariance sets without a GPU: the fused call, the stream and the multi predictor are declared and exported, refuse
bad arguments and fail loudly with no device, and the finalize kernel compiles without spills (csrc/gmm_full.hip, stream.cpp,
multi.cpp)."""
import ctypes as C

import numpy as np
import pytest

import fullcov_oracle as fo

NEW_SYMBOLS = ["sr_fullset_predict_pcm_batch", "sr_stream_create_full", "sr_multi_create_full"]


def test_new_symbols_exported_and_declared(built_lib):
    import test_abi_cpu
    from speaker_recognition_amd import _lib
    declared = test_abi_cpu.declared_symbols()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.EXT_SYMBOLS, name
        assert hasattr(raw, name), name


def test_argument_checks_come_before_the_device(built_lib):
    from speaker_recognition_amd.core import MfccExtractor
    ex = MfccExtractor(8000)
    assert not built_lib.sr_stream_create_full(ex._h, None, 6, 8000, 0, 1)
    assert b"SR_STREAM_GRAPH only" in built_lib.sr_last_error()
    assert not built_lib.sr_stream_create_full(ex._h, None, 6, 8000, 0, 0x100)
    assert b"bad arguments" in built_lib.sr_last_error()
    assert built_lib.sr_fullset_predict_pcm_batch(ex._h, None, None, 0, None, None) == -1
    assert b"null argument" in built_lib.sr_last_error()
    assert not built_lib.sr_multi_create_full(None, 0, 8000.0, 32.0, 16.0, 2048, 50, 13, 0.95, 15, 1)
    assert b"empty model list" in built_lib.sr_last_error()


def test_serving_stream_takes_model_sets_by_type(built_lib):
    from speaker_recognition_amd.core import MfccExtractor, ServingStream
    with pytest.raises(TypeError, match="FullSet"):
        ServingStream(MfccExtractor(8000), [1, 2], 6, 8000)


def test_entry_points_need_a_gpu(built_lib):
    """No CPU path: the multi predictor over full models raises 'no HIP device' without a GPU, an LPC order that is not built
    is refused first."""
    from speaker_recognition_amd import _lib, skgmm
    from speaker_recognition_amd.core import MultiPredictor
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    m = skgmm.GMM.from_arrays(*fo.random_model(np.random.default_rng(0), 2, 28))
    with pytest.raises(_lib.SRError, match="LPC order 14"):
        MultiPredictor.from_full([m], 16000, n_lpc=14)
    with pytest.raises(_lib.SRError, match="no HIP device"):
        MultiPredictor.from_full([m], 16000)
    with pytest.raises(_lib.SRError, match="no HIP device"):
        skgmm.FullSet([m])


def test_finalize_kernel_does_not_spill(built_lib):
    import test_abi_cpu
    res = test_abi_cpu._kernel_resources("gmm_full")
    names = [n for n in res if "fullcov_finalize_kernel" in n]
    assert len(names) == 1, sorted(res)
    assert res[names[0]]["scratch"] == 0, res[names[0]]

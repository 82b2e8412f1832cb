"""CPU-only tests of the 129..1024-state range: the limits the C ABI reports, the shapes it refuses before any device
call, and the fused-path choice of MultitrackHmm.  No GPU compute is needed (on a machine with one, the calls that
are accepted run and their handles are released)."""
import ctypes

import numpy as np

from tehmm_amd import _lib, build


def _lib_built():
    build.build()
    return _lib.load()


def _model_create(lib, N, K=2, S=4):
    lt = np.full((N, N), np.log(1.0 / N))
    pi = np.full(N, np.log(1.0 / N))
    lp = np.full((K, N, S), np.log(1.0 / S))
    h = ctypes.c_void_p()
    rc = lib.tehmm_model_create(N, K, S, lt.ctypes.data_as(_lib.f64p), pi.ctypes.data_as(_lib.f64p),
                                lp.ctypes.data_as(_lib.f64p), 1.0, None, ctypes.byref(h))
    if rc == 0:
        lib.tehmm_model_destroy(h)
    return rc


def _viterbi(lib, N, T=2):
    lt = np.full((N, N), np.log(1.0 / N))
    pi = np.full(N, np.log(1.0 / N))
    fr = np.zeros((T, N))
    path = np.zeros(T, dtype=np.int64)
    lp = ctypes.c_double(0.0)
    return lib.tehmm_viterbi(T, N, pi.ctypes.data_as(_lib.f64p), lt.ctypes.data_as(_lib.f64p), None,
                             fr.ctypes.data_as(_lib.f64p), path.ctypes.data_as(_lib.i64p), ctypes.byref(lp))


def test_state_limits():
    lib = _lib_built()
    assert lib.tehmm_max_states_any() == 1024
    assert lib.tehmm_max_states() == 128           # the fused / chunk-parallel limit stays
    assert lib.tehmm_abi_version() == 4


def test_more_than_1024_states_refused_before_any_device_call():
    lib = _lib_built()
    assert _model_create(lib, 1025) == -3
    assert b"1024" in lib.tehmm_last_error()
    assert _viterbi(lib, 1025) == -3
    assert b"1024" in lib.tehmm_last_error()


def test_129_to_1024_states_accepted():
    """Without a GPU these calls fail with a HIP error, never with TEHMM_ERR_UNSUPPORTED; with one they succeed."""
    lib = _lib_built()
    for N in (129, 200, 1024):
        assert _model_create(lib, N) != -3, N
        assert _viterbi(lib, N) != -3, N


def test_multitrack_hmm_fuses_200_states():
    from tehmm_amd.emission import IndependentMultinomialEmissionModel
    from tehmm_amd.hmm import MultitrackHmm
    h = MultitrackHmm(IndependentMultinomialEmissionModel(200, [3, 5]))
    a = np.array([[1, 2], [3, 5], [0, 1]], dtype=np.uint8)
    assert h._can_fuse([a])
    assert h._can_fuse([a.astype(np.uint16)])
    big = MultitrackHmm(IndependentMultinomialEmissionModel(1025, [3, 5]))
    assert not big._can_fuse([a])

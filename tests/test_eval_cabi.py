"""CPU: the evaluation-mode entries kpgnn_mlp_eval / kpgnn_bn_eval reject malformed descriptors before any device call
(no GPU is touched: every pointer is a dummy that is never dereferenced, the stream is NULL)."""
import ctypes

import pytest

A = 0x10000                                       # dummy, non-NULL, 16-B aligned: never dereferenced
EINVAL, ELIMIT = -1, -3


@pytest.fixture(scope="module")
def lib():
    from kp_gnn_amd import _lib, build
    build.build_all()
    return _lib.load()


def _running(r, *, var=True):
    r.gamma, r.beta, r.running_mean, r.eps = A, A, A, 1e-5
    r.running_var = A if var else None


def _mlp_desc(N=100, I=104, O=104):
    from kp_gnn_amd import _lib
    d = _lib.MlpEvalDesc()
    d.N, d.I, d.O = N, I, O
    d.x, d.x_stride, d.w0, d.b0, d.w3, d.b3, d.y, d.y_stride = A, I, A, A, A, A, A, O
    _running(d.bn1)
    _running(d.bn2)
    return d


def _bn_desc(N=100, C=104):
    from kp_gnn_amd import _lib
    d = _lib.BnEvalDesc()
    d.N, d.C = N, C
    d.x, d.x_stride, d.z, d.z_stride = A, C, A, C
    _running(d.bn)
    return d


def test_null_descriptors_are_rejected(lib):
    assert lib.kpgnn_mlp_eval(None, None) == EINVAL
    assert b"mlp_eval: NULL descriptor" in lib.kpgnn_last_error()
    assert lib.kpgnn_bn_eval(None, None) == EINVAL
    assert b"bn_eval: NULL descriptor" in lib.kpgnn_last_error()


@pytest.mark.parametrize("N", [0, -3])
def test_empty_row_counts_are_rejected(lib, N):
    assert lib.kpgnn_mlp_eval(ctypes.byref(_mlp_desc(N=N)), None) == EINVAL
    assert b"mlp_eval: bad N=" in lib.kpgnn_last_error()
    assert lib.kpgnn_bn_eval(ctypes.byref(_bn_desc(N=N)), None) == EINVAL
    assert b"bn_eval: bad N=" in lib.kpgnn_last_error()


@pytest.mark.parametrize("I,O,which", [(100, 104, 100), (104, 100, 100), (40, 32, 40), (256, 128, 256)])
def test_mlp_eval_refuses_widths_outside_the_unrolled_set(lib, I, O, which):
    """KPGNN_ELIMIT with the text every kernel of the fully unrolled k-loops gives (mfma_tile.h, MfmaWidths::refuse): the
    Python side keeps its other path for such a shape."""
    assert lib.kpgnn_mlp_eval(ctypes.byref(_mlp_desc(I=I, O=O)), None) == ELIMIT
    text = lib.kpgnn_last_error()
    assert b"mlp_eval" in text and (b"I=%d is not one of 32, 64, 96, 104, 128 (the k-loop is fully unrolled)" % which) in text


def test_the_refusal_text_is_the_one_linear_bn_gives(lib):
    from kp_gnn_amd import _lib
    assert lib.kpgnn_mlp_eval(ctypes.byref(_mlp_desc(I=100)), None) == ELIMIT
    ours = lib.kpgnn_last_error()
    d = _lib.LinearBnDesc()
    d.N, d.O, d.I = 100, 104, 100
    d.x, d.w, d.y = A, A, A
    assert lib.kpgnn_linear_bn(ctypes.byref(d), None) == ELIMIT
    theirs = lib.kpgnn_last_error()
    assert ours.split(b": ", 1)[1] == theirs.split(b": ", 1)[1]


def test_mlp_eval_refuses_unaligned_operands(lib):
    d = _mlp_desc()
    d.x = A + 4
    assert lib.kpgnn_mlp_eval(ctypes.byref(d), None) == ELIMIT
    d = _mlp_desc()
    d.residual, d.r_stride = A, 2 * 104 + 2
    assert lib.kpgnn_mlp_eval(ctypes.byref(d), None) == ELIMIT
    assert b"16-B aligned" in lib.kpgnn_last_error()


def test_missing_running_variance_is_rejected(lib):
    for which in ("bn1", "bn2", "outer"):
        d = _mlp_desc()
        _running(getattr(d, which), var=False)
        assert lib.kpgnn_mlp_eval(ctypes.byref(d), None) == EINVAL, which
        assert b"running_var" in lib.kpgnn_last_error()
    d = _bn_desc()
    _running(d.bn, var=False)
    assert lib.kpgnn_bn_eval(ctypes.byref(d), None) == EINVAL
    assert b"running_var" in lib.kpgnn_last_error()


def test_bn_eval_refuses_rows_wider_than_its_lanes(lib):
    assert lib.kpgnn_bn_eval(ctypes.byref(_bn_desc(C=260)), None) == ELIMIT
    assert b"bn_eval: C=260" in lib.kpgnn_last_error()

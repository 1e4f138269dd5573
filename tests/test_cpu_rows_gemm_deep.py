"""mhr_rows_gemm_deep validates its arguments on the host before any launch (no GPU needed): unsupported shapes, a misaligned
pointer and a leading dimension shorter than the row are refused with a message.  The pointers are dummies that a launch
would fault on."""
import pytest


@pytest.fixture(scope="module")
def dll():
    import __graft_entry__ as ge
    ge.build_hip_library()
    import mhr_amd  # noqa: F401
    from mhr_amd import lib
    return lib.load()


def test_rows_gemm_deep_supported_shapes(dll):
    for kn in (0, 1):
        assert dll.mhr_rows_gemm_deep_supported(1, 256, 1024, kn) == 1
        assert dll.mhr_rows_gemm_deep_supported(18432, 256, 1024, kn) == 1
        assert dll.mhr_rows_gemm_deep_supported(64, 128, 1024, kn) == 1
        assert dll.mhr_rows_gemm_deep_supported(64, 256, 256, kn) == 0
        assert dll.mhr_rows_gemm_deep_supported(64, 256, 2048, kn) == 0
        assert dll.mhr_rows_gemm_deep_supported(64, 200, 1024, kn) == 0
        assert dll.mhr_rows_gemm_deep_supported(0, 256, 1024, kn) == 0
    from mhr_amd import ops
    for M, N, K in ((1, 256, 1024), (64, 128, 1024), (64, 256, 256), (64, 200, 1024), (0, 256, 1024)):
        assert bool(ops.rows_gemm_deep_supported(M, N, K)) == bool(dll.mhr_rows_gemm_deep_supported(M, N, K, 0))


def test_rows_gemm_deep_rejects_bad_arguments_before_any_launch(dll):
    P = 4096

    def call(a=P, lda=1024, w=P, ldw=1024, kn=0, c=P, ldc=256, M=64, N=256, K=1024):
        return dll.mhr_rows_gemm_deep(a, lda, w, ldw, kn, c, ldc, M, N, K, None)

    assert call(a=None) == -1 and b"null" in dll.mhr_last_error()
    assert call(K=256) == -1 and b"K=256" in dll.mhr_last_error() and b"unsupported" in dll.mhr_last_error()
    assert call(N=264) == -1 and b"N=264" in dll.mhr_last_error()
    assert call(a=P + 8) == -1 and b"16-byte aligned" in dll.mhr_last_error()
    assert call(lda=1016) == -1 and b"leading dimensions" in dll.mhr_last_error()
    assert call(ldc=260) == -1 and b"leading dimensions" in dll.mhr_last_error()
    assert call(kn=1, ldw=128) == -1 and b"leading dimensions" in dll.mhr_last_error()

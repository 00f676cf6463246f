"""sbl_gemm2_rows_f32 without a GPU: its argument checks (they run on the host before any launch) and its qualifying rule
as tests/gemm_rows.py restates it, against expectations written by hand for the decoder forward's dual products."""
import ctypes

import pytest

import gemm_rows as G
import gemm_routes as R


def _call(M, N, K, a, lda, ldb, ldc, bias0, bias1, ws=None, ws_bytes=0):
    from sbl_for_multilingual_lip_reading_amd import _lib
    _lib.call("sbl_gemm2_rows_f32", M, N, K, a, a, lda, a, a, ldb, a, a, ldc, bias0, bias1, 0, ws, ws_bytes, None)


def test_bad_arguments_are_refused_on_the_host():
    """The addresses are host dummies: every call is refused before anything is dereferenced or launched."""
    from sbl_for_multilingual_lip_reading_amd import _lib
    buf = ctypes.create_string_buffer(64)
    a = (ctypes.addressof(buf) + 15) & ~15
    for M, N, K in ((0, 16, 16), (16, -1, 16), (16, 16, 0)):
        with pytest.raises(_lib.SblHipError, match="sbl_gemm2_rows_f32: non-positive dims"):
            _call(M, N, K, a, 16, 16, 16, None, None)
    with pytest.raises(_lib.SblHipError, match="sbl_gemm2_rows_f32: null operand / one-sided bias"):
        _call(16, 16, 16, None, 16, 16, 16, None, None)
    for b0, b1 in ((a, None), (None, a)):
        with pytest.raises(_lib.SblHipError, match="sbl_gemm2_rows_f32: null operand / one-sided bias"):
            _call(16, 16, 16, a, 16, 16, 16, b0, b1)
    for lda, ldb, ldc in ((12, 16, 16), (16, 15, 16), (16, 16, 8)):
        with pytest.raises(_lib.SblHipError, match="sbl_gemm2_rows_f32: leading dimension too small"):
            _call(16, 16, 16, a, lda, ldb, ldc, None, None)
    with pytest.raises(_lib.SblHipError, match="sbl_gemm2_rows_f32: workspace unaligned or < 16 KiB"):
        _call(16, 16, 16, a, 16, 16, 16, None, None, a, 64)


# (M, N, K) -> runs on 16x16 tiles?  The dual products of one training step at B = 32 (one to four decoding steps per stage,
# d_model 512, d_inner 2048, fused q/k/v 1536), workgroup counts of the 32x32 tiling worked out by hand:
DECODER_SHAPES = [
    ((32, 512, 2048), True),        # FFN2:  2 * 1 * 16 =  32
    ((64, 512, 2048), True),        #        2 * 2 * 16 =  64
    ((96, 512, 2048), True),        #        2 * 3 * 16 =  96
    ((128, 512, 2048), True),       #        2 * 4 * 16 = 128
    ((32, 512, 512), True),
    ((64, 512, 512), True),
    ((96, 512, 512), True),
    ((128, 512, 512), True),
    ((32, 1536, 512), True),        # q/k/v: 2 * 1 * 48 =  96
    ((64, 1536, 512), True),        #        2 * 2 * 48 = 192
    ((96, 1536, 512), False),       #        2 * 3 * 48 = 288
    ((32, 2048, 512), True),        # FFN1:  2 * 1 * 64 = 128
    ((64, 2048, 512), False),       #        2 * 2 * 64 = 256: not below 256
    ((256, 512, 2048), False),      #        2 * 8 * 16 = 256
    ((224, 512, 512), False),       #        2 * 7 * 16 = 224, but more than 128 rows
    ((160, 512, 2048), False),
    ((33, 2048, 512), False),       # one row over: 2 * 2 * 64
]


@pytest.mark.parametrize("shape,expect", DECODER_SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_rule_on_the_decoder_shapes(shape, expect):
    M, N, K = shape
    assert G.takes16(M, N, K, K, K, True) is expect
    assert G.noted_route(M, N, K, K, K, True) == ((9, 4, 8, 4 if K == 2048 else 2) if expect else (9, 0, 0, 0))


def test_rule_alignment_and_k():
    assert G.takes16(33, 40, 48, 48, 48, True)
    assert G.takes16(33, 40, 48, 52, 56, True)          # padded rows, still whole float4s
    assert not G.takes16(33, 40, 48, 48, 48, False)     # a pointer off a 16-byte boundary
    assert not G.takes16(33, 40, 48, 50, 48, True)      # lda % 4 != 0
    assert not G.takes16(33, 40, 48, 48, 49, True)
    assert not G.takes16(33, 40, 520, 520, 520, True)   # K % 16 == 8 (sbl_gemm2_f32 still takes its skinny kernel: K % 8 == 0)
    assert R.route_gemm2(33, 40, 520, 520, 520, True).family == "skinny"
    assert G.vu16(16) == (4, 2) and G.vu16(496) == (4, 2) and G.vu16(512) == (8, 2) and G.vu16(1008) == (8, 2) and G.vu16(1024) == (8, 4)
    assert G.same_sums(512) and G.same_sums(2048) and G.same_sums(64) and not G.same_sums(16) and not G.same_sums(48) and not G.same_sums(576)
    assert G.decode_route((9 << 24) | (4 << 20) | (8 << 10) | 4) == (9, 4, 8, 4)

"""The qualifying rule of sbl_gemm2_rows_f32 (csrc/gemm.hip: sbl_rows16_takes) restated in Python, and what the entry
point notes in sbl_profile_last_route().  Pure integer arithmetic, no torch, no GPU.  A call that does not qualify is
sbl_gemm2_f32 with the same arguments; gemm_routes.route_gemm2() says where that one lands."""
import gemm_routes as R

MAX_WGS32 = 256                     # tuning.h: sbl_rows16_max_wgs32
MAX_M = 128                         # tuning.h: sbl_rows16_max_m
DEEP_K = 1024                       # tuning.h: sbl_rows16_deep_k
ROUTE_FAMILY, TILE_16, TILE_FORWARDED = 9, 4, 0      # sbl_common.h: SBL_ROUTE_GEMM2_ROWS, SBL_ROUTE_TILE_16; 0 = forwarded


def takes16(M, N, K, lda, ldb, aligned):
    """True when the call runs on sbl_skinny16_gemm_kernel.  aligned: all four operand pointers are 16-byte aligned."""
    starved = 2 * R.cdiv(M, 32) * R.cdiv(N, 32) < MAX_WGS32 and M <= MAX_M
    return starved and K % 16 == 0 and aligned and lda % 4 == 0 and ldb % 4 == 0


def vu16(K):
    """skinny_gemm.h sbl_launch_skinny16: (V, U) by K - V ranges of K, the 32x32 kernel's NW; U groups per register stage."""
    return (R.skinny_nwu(K)[0], 4 if K >= DEEP_K else 2)


def same_sums(K):
    """The V ranges are the 32x32 kernel's own (multiples of 16 as well as of 8): the output is bit-identical to sbl_gemm2_f32's."""
    return K % (16 * vu16(K)[0]) == 0


def noted_route(M, N, K, lda, ldb, aligned):
    """(family, tile, V, U) the call leaves in sbl_profile_last_route()."""
    if takes16(M, N, K, lda, ldb, aligned):
        return (ROUTE_FAMILY, TILE_16) + vu16(K)
    return (ROUTE_FAMILY, TILE_FORWARDED, 0, 0)


def decode_route(code):
    """include/sbl_hip.h: (family << 24) | (tile << 20) | (TR << 10) | G."""
    return (code >> 24, (code >> 20) & 15, (code >> 10) & 1023, code & 1023)

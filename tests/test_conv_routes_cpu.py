"""tests/conv_routes.py against itself and against the promises of the kernels' headers (no GPU): the hand-written leaf
of every case, coverage of every reachable leaf, the tile facts of conv_patch.h / conv_patch_wgrad.h, and pwg_div."""
import numpy as np
import pytest

import conv_routes as R


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_route_equals_the_hand_written_leaf(case):
    for prec in R.PRECS:
        assert R.route(case, prec) == case.leaf[prec], prec


def test_case_table_reaches_every_leaf():
    hit = {R.leaf_key(c, c.leaf[p]) for c in R.CASES for p in R.PRECS}
    assert R.all_leaves() - hit == set()
    assert hit - R.all_leaves() == set()      # a leaf the table reaches and all_leaves() does not know is a mistake there


def test_route_codes_are_distinct():
    leaves = {c.leaf[p] for c in R.CASES for p in R.PRECS}
    codes = {}
    for leaf in leaves:
        codes.setdefault(R.route_code(leaf), set()).add((leaf.family, leaf.tile, leaf.tr, leaf.g))
    assert all(len(v) == 1 for v in codes.values())


def test_patch_forward_tiles_promised_by_conv_patch_h():
    for npl in (1, 2, 3):
        assert R.patch_tile(22, 22, npl) == (11, 1)
        assert R.patch_tile(28, 28, npl) == (7, 1)
        assert R.patch_tile(11, 11, npl) == (11, 2)
    for npl in (1, 2):
        assert R.patch_tile(6, 6, npl) == (6, 7)
        assert R.patch_tile(7, 7, npl) == (7, 5)
        assert R.patch_tile(4, 4, npl) == (4, 16)
        assert R.patch_tile(4, 5, npl) == (4, 12) and R.patch_tile(5, 4, npl) == (5, 12)
    assert R.patch_tile(3, 3, 1) == (3, 28)
    assert R.patch_tile(3, 3, 2) is None and R.patch_tile(3, 3, 3) is None
    for hw in ((6, 6), (7, 7), (4, 4), (4, 5), (5, 4), (9, 9), (8, 8)):
        assert R.patch_tile(hw[0], hw[1], 3) is None      # three planes: position-major
    assert R.patch_tile(9, 9, 2) == (9, 3) and R.patch_tile(8, 8, 2) == (8, 4)
    # the 64 bytes: three 9x9 images need (3 * 121 + 64) * 64 * 3 = 81984 bytes of the 81920
    assert (3 * 11 * 11 + 64) * R.CP_PIXB * 3 - R.CP_BUDGET == 64
    for prec in ("bf16x6", "bf16x3", "bf16"):
        assert R.route_fwd(prec, 2, 5, 9, 9, 64, 64, 3, 1).family == ("pm" if prec == "bf16x6" else "patch")


def test_patch_weight_gradient_tiles_promised_by_conv_patch_wgrad_h():
    for npl in (1, 2, 3):
        g = R.patch_wgrad_geom(1, 22, 22, npl)
        assert (g["TR"], g["G"], g["tpi"]) == (6, 1, 4)
        assert [min(6, 22 - t * 6) for t in range(g["tpi"])] == [6, 6, 6, 4]
        for H in (12, 24):      # even splits: 6 + 6 and 6 + 6 + 6 + 6
            g = R.patch_wgrad_geom(1, H, 22, npl)
            assert (g["TR"], g["G"], g["tpi"]) == (6, 1, H // 6) and H % g["TR"] == 0
        g = R.patch_wgrad_geom(1, 23, 22, npl)
        assert (g["TR"], g["tpi"]) == (6, 4) and [min(6, 23 - t * 6) for t in range(4)] == [6, 6, 6, 5]
        g = R.patch_wgrad_geom(4, 11, 11, npl)
        assert (g["TR"], g["G"], g["ntiles"]) == (11, 1, 4)
        g = R.patch_wgrad_geom(10, 6, 6, npl)
        assert (g["TR"], g["G"], g["ntiles"]) == (6, 3, 4)
        assert R.patch_wgrad_geom(1, 12, 3, npl) is None      # 2 images = 72 pixels < 80


def pwg_div(v, d):
    """conv_patch_wgrad.h pwg_div in float32: (int)(((float)v + 0.5f) * (1.0f / (float)d))."""
    r = np.float32(1.0) / np.float32(d)
    return ((v.astype(np.float32) + np.float32(0.5)) * r).astype(np.int32)


def test_pwg_div_is_exact_on_every_accepted_geometry():
    """The fp32-reciprocal division that builds the pixel -> patch-row table and the staging coordinates equals v // d for the
    four divisors sbl_conv_patch_wgrad_geom sets and every v below the larger of the two LDS images' row counts (the staging
    loops evaluate it for every row slot a thread owns, up to SBL_PWG_XQ * 768 / 16 = 240, before they test the row)."""
    seen = 0
    for npl in (1, 2, 3):
        for H in range(1, 65):
            for W in range(1, 65):
                g = R.patch_wgrad_geom(1, H, W, npl)
                if g is None:
                    continue
                seen += 1
                top = max(g["xrows"], g["dyrows"], R.PWG_XQ * R.PWG_THREADS // 16)
                v = np.arange(top, dtype=np.int64)
                for d in (g["PW"], g["PH"] * g["PW"], W, g["TR"] * W):
                    assert np.array_equal(pwg_div(v, d), (v // d).astype(np.int32)), (npl, H, W, d)
    assert seen > 1000

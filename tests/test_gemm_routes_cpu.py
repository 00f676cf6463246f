"""The route table of the dense GEMM tests (tests/gemm_routes.py), checked without a GPU: every case lands on the leaf
written next to it, the table reaches every reachable leaf, the integer data of the exact checks cannot round, and the
error bound of the rounded checks holds for a sequential fp32 emulation."""
import numpy as np
import pytest

import gemm_routes as R
from sbl_for_multilingual_lip_reading_amd import detfill

WS = {"full": R.WS_FULL, "short": R.WS_SHORT, None: None}


def dims(c):
    lda = (c.M if c.ta else c.K) + c.pa
    ldb = (c.K if c.tb else c.N) + c.pb
    return lda, ldb


def route_of(c):
    lda, ldb = dims(c)
    return R.route(c.ta, c.tb, c.M, c.N, c.K, lda, ldb, c.off == 0, "b" in c.epi, "r" in c.epi, "m" in c.epi,
                   "+" in c.epi, WS[c.ws])


def route2_of(c):
    return R.route_gemm2(c.M, c.N, c.K, c.K + c.pa, c.K + c.pb, c.off == 0, c.bias, c.relu, WS[c.ws])


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_case_lands_on_its_leaf(case):
    assert route_of(case) == case.leaf
    assert "c" not in case.epi or case.ta == 1            # a_colsum needs transA (the ABI refuses it otherwise)


@pytest.mark.parametrize("case", R.GEMM2_CASES, ids=lambda c: c.name)
def test_gemm2_case_lands_on_its_leaf(case):
    assert route2_of(case) == case.leaf


def test_every_reachable_leaf_has_a_case():
    want = R.all_leaves()
    have = {R.leaf_key(c.leaf) for c in R.CASES} | {R.leaf_key(c.leaf) for c in R.GEMM2_CASES}
    assert not (want - have), "leaves without a case: %s" % sorted(want - have, key=repr)
    assert not (have - want), "cases on leaves all_leaves() calls unreachable: %s" % sorted(have - want, key=repr)
    assert len(want) == 9 + 4 * (8 + 1 + 2) + 3 + 4


def test_every_epilogue_on_every_layout():
    """bias, ReLU, mask, += on each layout of each family; a_colsum on the skinny, 64x64 (split and unsplit, both
    transA layouts) and 128x128 kernels."""
    for fam, lays in (("skinny", ("nt", "nn", "tn")), ("tiled64", ("nt", "nn", "tn", "tt"))):
        for lay in lays:
            seen = "".join(c.epi for c in R.CASES if c.leaf.family == fam and c.leaf.layout == lay)
            assert set("brm+") <= set(seen), (fam, lay, seen)
    for red in ("none", "slabs", "atomics", "forced1"):
        for flag in "brm":
            if red == "atomics":
                continue                                   # atomics take the plain epilogue only
            assert any(flag in c.epi for c in R.CASES if c.leaf.family == "tiled64" and c.leaf.reduction == red), (red, flag)
    for fam, lay, split in (("skinny", "tn", False), ("tiled64", "tn", False), ("tiled64", "tn", True),
                            ("tiled64", "tt", False), ("tiled64", "tt", True), ("tiled128", "tn", False)):
        assert any("c" in c.epi for c in R.CASES
                   if c.leaf.family == fam and c.leaf.layout == lay and (c.leaf.splits > 1) == split), (fam, lay, split)


def test_integer_data_is_exact():
    """Operands, bias, previous C in [-3, 3]: every partial sum of every order stays an integer below 2^24."""
    for c in list(R.CASES) + list(R.GEMM2_CASES):
        assert 3 * 3 * c.K + 3 + 3 < 2 ** 24, c.name
    for c in R.CASES:                                      # a_colsum: K terms of magnitude <= 3 onto a previous value <= 3
        assert 3 * c.K + 3 < 2 ** 24


def fp32_sequential(A, B, bias, C0, splits):
    """C = A B^T the way a split-K launch adds it up, every addition rounded to fp32: `splits` contiguous K slices, each a
    chain of fused multiply-adds from zero (the product is exact in float64, the sum is rounded once to fp32 - up to a
    double rounding of relative size 2^-29), then the slices in order, then bias, then the previous C."""
    M, K = A.shape
    chunk = R.cdiv(K, splits)
    total = None
    for z in range(splits):
        acc = np.zeros((M, B.shape[0]), np.float32)
        for k in range(z * chunk, min(K, (z + 1) * chunk)):
            acc = (acc.astype(np.float64) + A[:, k, None].astype(np.float64) * B[None, :, k].astype(np.float64)).astype(np.float32)
        total = acc if total is None else (total + acc).astype(np.float32)
    if bias is not None:
        total = (total + bias[None, :]).astype(np.float32)
    if C0 is not None:
        total = (total + C0).astype(np.float32)
    return total


@pytest.mark.parametrize("M,N,K,splits,bias,acc", [(9, 7, 20, 1, True, False), (5, 11, 196, 3, True, True), (3, 4, 1540, 8, False, True)])
def test_bound_holds_for_sequential_fp32(M, N, K, splits, bias, acc):
    """(K + c) * U * (|A||B| + |bias| + |C0|) against float64, for the plainest summation order an fp32 kernel can use."""
    A, B = detfill.uniform("rc.A", (M, K)), detfill.uniform("rc.B", (N, K))
    b = detfill.uniform("rc.b", (N,)) if bias else None
    C0 = detfill.uniform("rc.C", (M, N)) if acc else None
    got = fp32_sequential(A, B, b, C0, splits)
    ref = A.astype(np.float64) @ B.astype(np.float64).T
    mag = np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64).T
    if bias:
        ref, mag = ref + b, mag + np.abs(b)
    if acc:
        ref, mag = ref + C0, mag + np.abs(C0)
    leaf = R.Leaf("tiled64", "nt", True, 4, splits, "slabs" if splits > 1 else "none")
    bound = (K + R.extra_roundings(leaf, bias, acc)) * R.U * mag
    err = np.abs(got.astype(np.float64) - ref)
    assert np.all(err <= bound)
    assert err.max() > 0                                   # the emulation does round: the check is not vacuous

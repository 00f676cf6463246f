"""The compact-to-full row map of the last decoder layer's "ends" layout (transformer/decoder.py: ends_rows) against a
brute-force enumeration.  Pure Python: no GPU, no library."""
import pytest

from sbl_for_multilingual_lip_reading_amd.transformer.decoder import ends_rows, stages_of

ML = 16
COINS = [False, True, False, False, True, True, False, False, False, True, False, True, False, False, False, False]      # mixed: runs of 1..4


def brute(n_seq, seg_lens, row0):
    """Walk every full row of the ragged batch in storage order and keep those at position 0 or L-1 of their sequence."""
    kept, r = [], row0
    for L in seg_lens:
        for _b in range(n_seq):
            for l in range(L):
                if l == 0 or l == L - 1:
                    kept.append(r)
                r += 1
    return kept


@pytest.mark.parametrize("B", [1, 3, 32])
def test_ends_rows_match_brute_force_for_all_steps_and_every_stage(B):
    rowoff = [B * t * (t + 1) // 2 for t in range(ML + 1)]
    whole = ends_rows(B, range(1, ML + 1))
    assert whole == brute(B, range(1, ML + 1), 0)
    assert len(whole) == B * 31 and len(set(whole)) == len(whole) and whole == sorted(whole)
    # (s, b, k) order: compact row of segment t, sequence b, k stands for rowoff[t] + b*L + k*(L-1)
    c = 0
    for t in range(ML):
        L = t + 1
        for b in range(B):
            for k in range(min(2, L)):
                assert whole[c] == rowoff[t] + b * L + k * (L - 1)
                c += 1
    # every stage of a mixed coin pattern maps its own rows, and the stages' maps concatenate to the whole batch's
    stages = stages_of(COINS, ML)
    assert 1 < len(stages) < ML and stages[0] == (0, 1)
    cat = []
    for i0, i1 in stages:
        seg = range(i0 + 1, i1 + 2)
        part = ends_rows(B, seg, rowoff[i0])
        assert part == brute(B, seg, rowoff[i0])
        assert len(part) == B * sum(min(2, L) for L in seg)
        cat += part
    assert cat == whole


def test_ends_rows_single_step_stages():
    """All-own-argmax coins: 16 one-segment stages, the L = 1 step alone among them (one row per sequence that is both ends)."""
    B = 3
    assert ends_rows(B, [1]) == [0, 1, 2]
    assert ends_rows(B, [1], 7) == [7, 8, 9]
    assert ends_rows(B, [2]) == [0, 1, 2, 3, 4, 5]
    assert ends_rows(B, [5], 10) == [10, 14, 15, 19, 20, 24]
    for i0, i1 in stages_of([True] * ML, ML):
        assert i0 == i1
        assert ends_rows(B, [i0 + 1], 100) == brute(B, [i0 + 1], 100)

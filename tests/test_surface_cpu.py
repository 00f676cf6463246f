"""CPU checks of the host-side model surface that no compute test sees: the seeded initialisation (every RNG draw of
the constructors, in order), the positional-encoding table and the mask / padding helpers."""
import numpy as np
import torch

from conftest import load_golden, maxdiff


def _check_init(g, prefix, sd):
    keys = [str(k) for k in g[prefix + "keys"]]
    assert list(sd.keys()) == keys
    for i, (k, v) in enumerate(sd.items()):
        v = v.detach().double()
        flat = v.reshape(-1)[:16].numpy()
        assert np.allclose(flat, g[prefix + "head"][i, :flat.size], rtol=0.0, atol=1e-6), k
        scale = max(float(g[prefix + "abs_sum"][i]), 1.0)
        assert abs(float(v.abs().sum()) - g[prefix + "abs_sum"][i]) <= 1e-6 * scale, k
        assert abs(float(v.sum()) - g[prefix + "sum"][i]) <= 1e-6 * scale, k


def test_seeded_init_matches_reference():
    """tests/golden/init_seeded.npz holds the reference's own models built under the same seeds: a different number,
    order, size or scale of RNG draws anywhere in the constructors moves these values by O(1)."""
    from sbl_for_multilingual_lip_reading_amd.transformer.decoder import Decoder
    from sbl_for_multilingual_lip_reading_amd.transformer.encoder import Encoder
    from sbl_for_multilingual_lip_reading_amd.transformer.transformer import Transformer
    from sbl_for_multilingual_lip_reading_amd.transformer.video_frontend import Lipreading
    g = load_golden("init_seeded.npz")
    torch.manual_seed(0)
    m = Transformer(Encoder(512, 2, 8, 64, 64, 512, 2048), Decoder(0, 1, 58, 512, 2, 8, 64, 64, 512, 2048), None)
    _check_init(g, "transformer.", m.state_dict())
    torch.manual_seed(1)
    _check_init(g, "lipreading.", Lipreading().state_dict())


def test_positional_encoding_table(golden_modules):
    from sbl_for_multilingual_lip_reading_amd.transformer.module import PositionalEncoding
    pe = PositionalEncoding(512).pe
    assert pe.shape == (1, 5000, 512) and pe.dtype == torch.float32
    assert maxdiff(pe[0, :64], golden_modules["pe"]) <= 63 * 2.0 ** -24 + 2 * 2.0 ** -24


def test_mask_and_pad_helpers():
    from sbl_for_multilingual_lip_reading_amd.transformer import utils as U
    x = torch.zeros(3, 4, 2, dtype=torch.float64)           # ragged batch: lengths 4, 1, 2 of T = 4
    lengths = [4, 1, 2]
    valid = [[1, 1, 1, 1], [1, 0, 0, 0], [1, 1, 0, 0]]

    m = U.get_non_pad_mask(x, input_lengths=lengths)
    assert m.dtype == torch.float64 and m.shape == (3, 4, 1)
    assert m[..., 0].tolist() == valid
    ids = torch.tensor([[5, 7, 0], [0, 0, 0]])
    m = U.get_non_pad_mask(ids, pad_idx=0)
    assert m.dtype == torch.float32 and m.shape == (2, 3, 1)
    assert m[..., 0].tolist() == [[1, 1, 0], [0, 0, 0]]

    a = U.get_attn_pad_mask(x, torch.tensor(lengths), 5)
    assert a.dtype == torch.bool and a.shape == (3, 5, 4) and a.stride(1) == 0
    assert a[:, 0].tolist() == [[v == 0 for v in row] for row in valid]
    assert torch.equal(a, a[:, :1].expand(-1, 5, -1))

    s = U.get_subsequent_mask(torch.zeros(2, 3, dtype=torch.long))
    assert s.dtype == torch.uint8 and s.shape == (2, 3, 3) and s.stride(0) == 0
    assert s[1].tolist() == [[0, 1, 1], [0, 0, 1], [0, 0, 0]]

    k = U.get_attn_key_pad_mask(torch.tensor([[3, 1, 1], [1, 2, 4]]), torch.zeros(2, 2), 1)
    assert k.dtype == torch.bool and k.shape == (2, 2, 3) and k.stride(1) == 0
    assert k[:, 1].tolist() == [[False, True, True], [True, False, False]]

    p = U.pad_list([torch.tensor([4, 5, 6]), torch.tensor([7])], -1)
    assert p.dtype == torch.long and p.shape == (2, 16)
    assert p[0].tolist() == [4, 5, 6] + [-1] * 13 and p[1].tolist() == [7] + [-1] * 15
    p = U.pad_list([torch.ones(2, 3), torch.full((1, 3), 2.0)], 0.5)
    assert p.shape == (2, 16, 3) and p[1, 0].tolist() == [2.0] * 3 and p[1, 1:].eq(0.5).all() and p[0, 2:].eq(0.5).all()

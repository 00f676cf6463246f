"""CPU-side checks of the drop-in boundary: the C-ABI library loads, exports every symbol include/sbl_hip.h
declares (and the ctypes table binds exactly those), the Python mirror keeps the reference's class surface and
state-dict keys, and the product path refuses to run without a GPU instead of falling back.  No compute calls."""
import os
import re
import subprocess
import sys

import pytest

from conftest import load_golden
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sbl_hip.h")


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sbl_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from sbl_for_multilingual_lip_reading_amd import _lib
    lib = _lib.load()
    assert lib.sbl_abi_version() == 1
    names = _declared()
    assert len(names) >= 36
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sbl_[a-z0-9_]+)", out))
    missing = [n for n in names if n not in exported]
    assert not missing, missing
    # ctypes table == header (minus the two non-int helpers)
    helpers = ("sbl_last_error", "sbl_abi_version", "sbl_profile_begin", "sbl_profile_end", "sbl_profile_last_slot",
               "sbl_profile_last_kernel", "sbl_profile_last_route", "sbl_profile_used", "sbl_wgrad_group_table_bytes",
               "sbl_get_matmul_precision")      # bound by hand in _lib.load()
    assert sorted(_lib.SIGNATURES) == sorted(n for n in names if n not in helpers)
    for h in helpers:
        assert hasattr(lib, h)


def test_ctypes_arity_matches_header():
    from sbl_for_multilingual_lip_reading_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, argtypes in _lib.SIGNATURES.items():
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
        assert m, name
        nargs = len([a for a in m.group(1).split(",") if a.strip()])
        assert nargs == len(argtypes), (name, nargs, len(argtypes))


def test_invalid_arguments_are_rejected_on_the_host():
    """Shape / pointer validation happens before any launch, so this is safe without a GPU."""
    from sbl_for_multilingual_lip_reading_amd import _lib
    with pytest.raises(_lib.SblHipError, match="non-positive dims"):
        _lib.call("sbl_gemm_f32", 0, 1, 0, 4, 4, None, 4, None, 4, None, 4, None, 0, None, 0, 0, None, None, 0, None)
    with pytest.raises(_lib.SblHipError, match="Lq,Lk <= 64"):
        _lib.call("sbl_attention_fwd", None, 64, None, 64, None, 64, None, 64, None, 0, None, 1, 1, 65, 4, 0.125, 0.0,
                  None, 0, None)
    with pytest.raises(_lib.SblHipError, match="sbl_set_matmul_precision: 2"):
        _lib.call("sbl_set_matmul_precision", 2)
    assert _lib.load().sbl_get_matmul_precision() == 0      # the library starts in exact-fp32 mode
    with pytest.raises(_lib.SblHipError, match="D=256"):
        _lib.call("sbl_add_layernorm_fwd", None, None, None, None, None, None, None, 4, 256, 1e-5, 0.0, None, 0, None)


def test_bn_bwd_reduce_refuses_channel_counts_its_combine_cannot_cover():
    """With a workspace the last block of sbl_bn_bwd_reduce combines the partials with G = 256 / (C/2) block groups; at
    C = 1024 (which 'C/4 divides 256' admits) G is 0 and its loop never advances, so the host refuses C > 512 before any
    launch.  The addresses are host dummies: nothing is dereferenced before the refusal.  C = 512 and C = 4 pass the
    range check and are stopped by a later argument (a 1-byte workspace), so nothing is launched here either."""
    import ctypes
    from sbl_for_multilingual_lip_reading_amd import _lib
    buf = ctypes.create_string_buffer(64)
    a = (ctypes.addressof(buf) + 15) & ~15
    with pytest.raises(_lib.SblHipError, match="C=1024"):
        _lib.call("sbl_bn_bwd_reduce", a, a, a, a, a, a, 8, 1024, 1, a, 16 << 20, None)
    with pytest.raises(_lib.SblHipError, match="C=1024"):
        _lib.call("sbl_bn_bwd_reduce", a, a, a, a, a, a, 8, 1024, 0, None, 0, None)
    for C in (512, 4):
        with pytest.raises(_lib.SblHipError, match="workspace unaligned or < 16 KiB"):
            _lib.call("sbl_bn_bwd_reduce", a, a, a, a, a, a, 8, C, 1, a, 1, None)


def test_state_dict_surface_matches_reference():
    from oracle import sbl_oracle as O
    from sbl_for_multilingual_lip_reading_amd.transformer.decoder import Decoder
    from sbl_for_multilingual_lip_reading_amd.transformer.encoder import Encoder
    from sbl_for_multilingual_lip_reading_amd.transformer.transformer import Transformer
    m = Transformer(Encoder(512, 6, 8, 64, 64, 512, 2048), Decoder(0, 1, 58, 512, 6, 8, 64, 64, 512, 2048), None)
    sd = m.state_dict()
    assert len(sd) == 537                                   # SURVEY.md 3.5 [probe]
    assert sum(p.numel() for p in m.parameters()) == 80898240
    shapes = O.state_dict_shapes(6, 6)
    got = {k: tuple(v.shape) for k, v in sd.items() if not k.endswith(".pe")}
    assert got == {k: tuple(v) for k, v in shapes.items()}
    # ... and against the REFERENCE's own model (tests/golden/state_dict_keys.npz, written by oracle/make_goldens.py from
    # /root/reference): every key, shape and dtype, parameters and buffers alike, in the reference's registration order
    ref = load_golden("state_dict_keys.npz")
    assert sorted(sd.keys()) == [str(k) for k in ref["keys"]]
    for k, shp, dt in zip(ref["keys"], ref["shapes"], ref["dtypes"]):
        assert ",".join(str(d) for d in sd[str(k)].shape) == str(shp) and str(sd[str(k)].dtype) == str(dt), str(k)
    assert [n for n, _ in m.named_parameters()] == [str(n) for n in ref["param_names"]]
    assert [n for n, _ in m.named_buffers()] == [str(n) for n in ref["buffer_names"]]
    assert tuple(sd["encoder.positional_encoding.pe"].shape) == (1, 5000, 512)
    # q/k/v projection weights are adjacent rows of one fused buffer after _fuse()
    mha = m.encoder.layer_stack[0].slf_attn
    mha._fuse()
    w = (mha.w_qs.weight, mha.w_ks.weight, mha.w_vs.weight)
    assert w[1].data_ptr() == w[0].data_ptr() + w[0].numel() * 4 and w[2].data_ptr() == w[1].data_ptr() + w[1].numel() * 4
    # the module stays picklable (SBL/utils.py:22-33 torch.save(model))
    import io
    import pickle
    pickle.dumps(m.state_dict()["decoder.tgt_word_prj_l2r.weight"])
    buf = io.BytesIO()
    torch.save(m.state_dict(), buf)


def test_dropin_top_level_names():
    """With the package directory on sys.path the reference's own import lines work (SBL/train.py:11-19)."""
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "from config import device, print_freq, sos_id, eos_id, word_number, p, vocab_size\n"
        "from transformer.decoder import Decoder\n"
        "from transformer.encoder import Encoder\n"
        "from transformer.loss import cal_performance\n"
        "from transformer.optimizer import TransformerOptimizer\n"
        "from transformer.transformer import Transformer\n"
        "assert (sos_id, eos_id, vocab_size) == (0, 1, 58)\n"
        "print('ok')\n" % os.path.join(ROOT, "sbl_for_multilingual_lip_reading_amd"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/tmp")
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


def test_no_cpu_fallback():
    """CPU tensors must be refused, not silently computed by torch."""
    from sbl_for_multilingual_lip_reading_amd import _lib, ops
    with pytest.raises(_lib.SblHipError, match="no CPU path"):
        ops.linear(torch.zeros(2, 4), torch.zeros(3, 4))


def test_preprocess_and_noam_match_golden(golden_modules):
    import numpy as np
    from sbl_for_multilingual_lip_reading_amd.transformer.decoder import Decoder
    from sbl_for_multilingual_lip_reading_amd.transformer.optimizer import TransformerOptimizer
    g = golden_modules
    dec = Decoder(0, 1, 58, 512, 1, 8, 64, 64, 512, 2048)
    yi, yo = dec.preprocess(torch.from_numpy(g["prep.tgt"]))
    assert np.array_equal(yi.numpy(), g["prep.ys_in"]) and np.array_equal(yo.numpy(), g["prep.ys_out"])
    # interior IGNORE_IDs are stripped too (y[y != IGNORE_ID], decoder.py:66)
    t = torch.tensor([[5, -1, 7, -1, -1, 9, -1, -1, -1, -1, -1, -1, -1, -1]])
    yi, yo = dec.preprocess(t)
    assert yi[0, :5].tolist() == [0, 5, 7, 9, 1] and yo[0, :4].tolist() == [5, 7, 9, 1]
    p = torch.nn.Parameter(torch.zeros(3))
    opt = TransformerOptimizer(torch.optim.Adam([p], lr=1e-3, betas=(0.9, 0.98), eps=1e-9))
    for s in range(3):
        opt._update_lr()
        assert abs(opt.lr - float(g["opt.lrs"][s])) < 1e-15

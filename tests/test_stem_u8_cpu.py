"""CPU-side checks of the uint8 -> stem direct feed (sbl_stem_conv_fwd_u8 / sbl_stem_wgrad_u8, ops.RawClips): the two entry
points are declared, bound and exported; bad arguments are refused on the host before any launch; RawClips validates what
it is given and does not compute without a GPU.  No kernel runs here."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sbl_hip.h")
NEW = ("sbl_stem_conv_fwd_u8", "sbl_stem_wgrad_u8")


def test_new_entry_points_are_declared_bound_and_exported():
    from sbl_for_multilingual_lip_reading_amd import _lib
    lib = _lib.load()
    assert lib.sbl_abi_version() == 1                      # additions do not bump the ABI version
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sbl_[a-z0-9_]+)", out))
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
        assert m, "%s is not declared in include/sbl_hip.h" % name
        nargs = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs, (name, nargs)
        assert name in exported, name
    # the raw entry points take the fp32 ones' arguments with the eight source arguments in place of x, T, H, W -> 7 dims
    assert len(_lib.SIGNATURES["sbl_stem_conv_fwd_u8"]) == len(_lib.SIGNATURES["sbl_stem_conv_fwd"]) - 1 - 4 + 6 + 7
    assert len(_lib.SIGNATURES["sbl_stem_wgrad_u8"]) == len(_lib.SIGNATURES["sbl_stem_wgrad"]) - 1 - 4 + 6 + 7


def _fwd(ptrs=None, dims=(2, 6, 32, 32, 6, 24, 24)):
    """sbl_stem_conv_fwd_u8 with fake non-null pointers: every case below is refused before anything is dereferenced."""
    from sbl_for_multilingual_lip_reading_amd import _lib
    p = [0x1000] * 9 if ptrs is None else ptrs
    _lib.call("sbl_stem_conv_fwd_u8", *p, *dims, None)


def _wgrad(ptrs=None, dims=(2, 6, 32, 32, 6, 24, 24)):
    from sbl_for_multilingual_lip_reading_amd import _lib
    p = [0x1000] * 17 if ptrs is None else ptrs
    _lib.call("sbl_stem_wgrad_u8", *p, *dims, None)


@pytest.mark.parametrize("fn,nptr", [(_fwd, 9), (_wgrad, 17)])
def test_invalid_arguments_are_rejected_on_the_host(fn, nptr):
    from sbl_for_multilingual_lip_reading_amd import _lib
    lib = _lib.load()
    for null_at in (0, 1, 5, nptr - 1):                    # frames, table, src_frame, the last output
        ptrs = [0x1000] * nptr
        ptrs[null_at] = None
        with pytest.raises(_lib.SblHipError, match="null pointer"):
            fn(ptrs)
        assert b"null pointer" in lib.sbl_last_error()
    with pytest.raises(_lib.SblHipError, match="bad dims"):                # Hc > Hin
        fn(dims=(2, 6, 32, 32, 6, 40, 24))
    with pytest.raises(_lib.SblHipError, match="bad dims"):                # Wc > Win
        fn(dims=(2, 6, 32, 32, 6, 24, 40))
    with pytest.raises(_lib.SblHipError, match="bad dims"):                # Tout <= 0
        fn(dims=(2, 6, 32, 32, 0, 24, 24))
    with pytest.raises(_lib.SblHipError, match="bad dims"):
        fn(dims=(2, 6, 32, 32, -3, 24, 24))
    # the stem's own rule on the logical clip (H, W multiples of 4, at least 8), as for the fp32 source today
    with pytest.raises(_lib.SblHipError, match="multiples of 4"):
        _lib.call("sbl_stem_conv_fwd", 0x1000, 0x1000, 0x1000, 0x1000, 2, 6, 23, 24, None)
    for hc, wc in ((23, 24), (24, 23), (22, 24), (4, 24)):
        with pytest.raises(_lib.SblHipError, match="multiples of 4"):
            fn(dims=(2, 6, 32, 32, 6, hc, wc))
        assert b"multiples of 4" in lib.sbl_last_error()
    with pytest.raises(_lib.SblHipError, match="too large"):               # 32-bit element offsets into the frames
        fn(dims=(4096, 64, 96, 96, 6, 88, 88))


def _good(N=3, Tin=5, Hin=32, Win=40, Tout=6, crop=(24, 32)):
    g = torch.Generator().manual_seed(1)
    frames = torch.randint(0, 256, (N, Tin, Hin, Win), generator=g).to(torch.uint8)
    y1 = torch.randint(0, Hin - crop[0] + 1, (N,), generator=g).int()
    x1 = torch.randint(0, Win - crop[1] + 1, (N,), generator=g).int()
    flip = torch.tensor([1, 0, 1][:N]).int()
    src = torch.randint(-1, Tin, (N, Tout), generator=g).int()
    return dict(frames_u8=frames, y1=y1, x1=x1, flip=flip, src_frame=src, crop=crop)


def test_rawclips_shape_and_fields():
    from sbl_for_multilingual_lip_reading_amd import ops
    a = _good()
    raw = ops.RawClips(**a)
    assert tuple(raw.shape) == (3, 6, 24, 32) and raw.dim() == 4 and raw.size(1) == 6
    assert raw.frames_u8 is a["frames_u8"] and raw.src_frame is a["src_frame"] and raw.crop == (24, 32)
    assert (raw.mean, raw.std) == (0.413621, 0.1700239)
    with pytest.raises(AttributeError):
        raw.crop = (8, 8)
    again = raw.to("cpu")
    assert isinstance(again, ops.RawClips) and tuple(again.shape) == tuple(raw.shape)
    # extreme but legal origins
    a = _good()
    a["y1"][:] = 32 - 24
    a["x1"][:] = 0
    ops.RawClips(**a)


def test_rawclips_refuses_bad_tensors():
    from sbl_for_multilingual_lip_reading_amd import ops
    for key, bad in (("frames_u8", lambda t: t.float()), ("y1", lambda t: t.long()), ("x1", lambda t: t.float()),
                     ("flip", lambda t: t.bool()), ("src_frame", lambda t: t.long())):
        a = _good()
        a[key] = bad(a[key])
        with pytest.raises(TypeError, match=key):
            ops.RawClips(**a)
    for key, bad in (("frames_u8", lambda t: t[0]), ("frames_u8", lambda t: t.unsqueeze(1)), ("y1", lambda t: t[:2]),
                     ("x1", lambda t: t.view(3, 1)), ("flip", lambda t: t[:1]), ("src_frame", lambda t: t[0]),
                     ("src_frame", lambda t: t[:2])):
        a = _good()
        a[key] = bad(a[key])
        with pytest.raises(ValueError, match=key):
            ops.RawClips(**a)
    a = _good()
    a["frames_u8"] = a["frames_u8"].transpose(2, 3).contiguous().transpose(2, 3)       # right shape, wrong strides
    with pytest.raises(ValueError, match="contiguous"):
        ops.RawClips(**a)
    a = _good()
    a["src_frame"] = a["src_frame"].t().contiguous().t()
    with pytest.raises(ValueError, match="contiguous"):
        ops.RawClips(**a)
    a = _good()
    a["crop"] = (40, 32)                                                               # crop larger than the frames
    with pytest.raises(ValueError, match="crop"):
        ops.RawClips(**a)


def test_rawclips_checks_ranges_of_host_indices():
    from sbl_for_multilingual_lip_reading_amd import ops
    for key, value in (("y1", -1), ("y1", 32 - 24 + 1), ("x1", -1), ("x1", 40 - 32 + 1), ("src_frame", 5)):
        a = _good()
        a[key].view(-1)[1] = value
        with pytest.raises(ValueError, match=key):
            ops.RawClips(**a)
    a = _good()
    a["src_frame"][:] = -1                                  # any negative entry is a zero frame
    a["src_frame"][0, 0] = -7
    ops.RawClips(**a)


def test_rawclips_does_not_compute_on_the_cpu():
    """No CPU fallback (test_abi_cpu.test_no_cpu_fallback states the policy): materialising and the stem itself refuse."""
    from sbl_for_multilingual_lip_reading_amd import _lib, ops
    raw = ops.RawClips(**_good())
    with pytest.raises(_lib.SblHipError, match="no CPU path"):
        raw.materialize()
    w = torch.zeros(64, 1, 5, 7, 7)
    with pytest.raises(_lib.SblHipError, match="no CPU path"):
        ops.StemFn.apply(raw, w, torch.ones(64), torch.zeros(64), torch.zeros(64), torch.ones(64), False, 0.1, 1e-5)

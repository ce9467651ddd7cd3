"""The two launches of flip test-time augmentation (csrc/tta.hip) against their definitions, bit for bit: the staging entries against the
existing conversion entries on the image and on torch.flip(image, W); zsg_tta_flip_merge against tests/tta_ref.merge_ref (bit patterns,
NaN matched as NaN).  Canary words in front of and behind every output; argument errors return -1 and write nothing."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tta_ref as R  # noqa: E402

CANARY = -1234.5
PAD = 64                      # floats in front of and behind an output (the front pad keeps the output 16-byte aligned)
SHAPES = [(1, 1, 1), (2, 3, 5), (3, 4, 7), (2, 5, 8), (2, 17, 33)]
LEVELS = {"one": [(1, 1)], "tiny": [(3, 4), (1, 1)], "odd": [(7, 5), (4, 3), (2, 1)]}


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib
    return _lib


def guarded(n):
    whole = torch.full((n + 2 * PAD,), CANARY, device="cuda")
    return whole, whole[PAD:PAD + n]


def guards_intact(whole, n):
    return bool((whole[:PAD] == CANARY).all()) and bool((whole[PAD + n:] == CANARY).all())


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_staging_is_the_plain_conversion_of_the_image_and_of_its_mirror(L, u8, B, H, W):
    lib, check, sp = L.lib, L.check, L.stream_ptr
    g = torch.Generator().manual_seed(B * 1000 + H * 37 + W)
    if u8:
        img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).cuda()
        flipped = torch.flip(img, [2]).contiguous()
    else:
        img = torch.rand(B, 3, H, W, generator=g).cuda()
        flipped = torch.flip(img, [3]).contiguous()

    def plain(x):
        out = torch.full((B, H, W, 4), CANARY, device="cuda")
        if u8:
            check(lib.zsg_u8hwc_to_nhwc4(x.data_ptr(), B * H * W, out.data_ptr(), sp()), "u8hwc_to_nhwc4")
        else:
            check(lib.zsg_nchw_to_nhwc4(x.data_ptr(), B, 3, H, W, out.data_ptr(), sp()), "nchw_to_nhwc4")
        return out
    n = 2 * B * H * W * 4
    whole, out = guarded(n)
    fn = lib.zsg_tta_flip_stage_u8 if u8 else lib.zsg_tta_flip_stage_f32
    check(fn(img.data_ptr(), B, H, W, out.data_ptr(), sp()), "tta_flip_stage")
    torch.cuda.synchronize()
    got = out.view(2 * B, H, W, 4)
    assert torch.equal(bits(got[:B]), bits(plain(img))), "rows 0..B-1: the batch as given"
    assert torch.equal(bits(got[B:]), bits(plain(flipped))), "rows B..2B-1: the batch mirrored along W"
    assert guards_intact(whole, n)
    assert bool((got[..., 3] == 0).all()) and not bool((got == CANARY).any())


def test_staging_argument_errors_write_nothing(L):
    lib = L.lib
    img = torch.zeros(2, 3, 4, 5, device="cuda")
    n = 2 * 2 * 4 * 5 * 4
    whole, out = guarded(n)
    for fn in (lib.zsg_tta_flip_stage_u8, lib.zsg_tta_flip_stage_f32):
        assert fn(None, 2, 4, 5, out.data_ptr(), L.stream_ptr()) == -1
        assert fn(img.data_ptr(), 2, 4, 5, None, L.stream_ptr()) == -1
        assert fn(img.data_ptr(), 0, 4, 5, out.data_ptr(), L.stream_ptr()) == -1
        assert fn(img.data_ptr(), 2, 0, 5, out.data_ptr(), L.stream_ptr()) == -1
        assert fn(img.data_ptr(), 2, 4, -1, out.data_ptr(), L.stream_ptr()) == -1
        assert fn(img.data_ptr(), 2, 4, 5, out.data_ptr() + 4, L.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert bool((whole == CANARY).all())


def special_values(shape, seed):
    """random data salted with +-0, +-inf, NaN, denormals, the largest finite values (inf - inf, inf + inf, overflow, 0.5 * denormal)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape).astype(np.float32)
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.1754942e-38, -5.9e-39, 3.4028235e38, -3.4028235e38, 1.0, -1.0], np.float32)
    flat = x.reshape(-1)
    where = rng.random(flat.shape[0]) < 0.5
    flat[where] = sp[rng.integers(0, len(sp), int(where.sum()))]
    return x


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [9, 1])
@pytest.mark.parametrize("name", sorted(LEVELS))
@pytest.mark.parametrize("data", ["random", "special"])
def test_merge_equals_merge_ref_bit_for_bit(L, data, name, n, B):
    sizes = LEVELS[name]
    lv = R.level_table(sizes, n)
    A = int(lv[-1, 0] + lv[-1, 1] * lv[-1, 2] * lv[-1, 3])
    seed = 100 * B + 10 * n + len(sizes)
    x = np.random.default_rng(seed).standard_normal((2 * B, A, 5)).astype(np.float32) if data == "random" else special_values((2 * B, A, 5), seed)
    want = R.merge_ref(x, sizes, n)
    src = torch.from_numpy(x).cuda()
    whole, out = guarded(B * A * 5)
    L.check(L.lib.zsg_tta_flip_merge(src.data_ptr(), B, A, lv.ctypes.data, lv.shape[0], out.data_ptr(), L.stream_ptr()), "tta_flip_merge")
    torch.cuda.synchronize()
    got = out.view(B, A, 5).cpu().numpy()
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "NaN where the reference has NaN, nowhere else"
    assert np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn])
    if data == "special" and want.size >= 500:      # (the salt reaches every class of result once there are enough elements)
        assert wn.any() and np.isinf(want).any() and (want == 0).any()
    assert guards_intact(whole, B * A * 5)
    assert torch.equal(bits(src), torch.from_numpy(x).view(torch.int32)), "the input is not written"


def test_merge_argument_errors_write_nothing(L):
    lib, sp = L.lib, L.stream_ptr
    sizes, n, B = LEVELS["tiny"], 9, 2
    lv = R.level_table(sizes, n)
    A = 13 * 9
    src = torch.randn(2 * B, A, 5, device="cuda")
    whole, out = guarded(B * A * 5)
    before = src.clone()

    def call(s=src.data_ptr(), b=B, a=A, t=lv, l=2, o=out.data_ptr()):
        return lib.zsg_tta_flip_merge(s, b, a, t.ctypes.data if t is not None else None, l, o, sp())
    assert call(a=A + 9) == -1 and call(a=A - 9) == -1 and call(l=1) == -1, "levels that do not sum to A"
    nine = np.array([(i, 1, 1, 1) for i in range(9)], np.int32)
    assert call(a=9, t=nine, l=9) == -1 and b"L=9" in lib.zsg_last_error()
    assert call(s=None) == -1 and call(o=None) == -1 and call(t=None) == -1
    gap = lv.copy()
    gap[1, 0] += 1
    assert call(t=gap) == -1
    zero = lv.copy()
    zero[1, 2] = 0
    assert call(t=zero) == -1
    assert call(b=0) == -1 and call(l=0) == -1
    # an aliased out: on the input, inside it, ending inside it
    assert call(o=src.data_ptr()) == -1 and b"overlap" in lib.zsg_last_error()
    assert call(o=src.data_ptr() + B * A * 20) == -1 and call(o=src.data_ptr() - B * A * 20 + 4) == -1
    torch.cuda.synchronize()
    assert bool((whole == CANARY).all()) and torch.equal(bits(src), bits(before))
    # ... and the good call still works
    L.check(call(), "tta_flip_merge")
    torch.cuda.synchronize()
    assert np.array_equal(out.view(B, A, 5).cpu().numpy().view(np.uint32), R.merge_ref(before.cpu().numpy(), sizes, n).view(np.uint32))

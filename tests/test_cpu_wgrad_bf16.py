"""wgrad_dtype = "bf16" without a GPU: the cfg key and its validation where the net is built, ZSGNet.wgrad_precision, the training plan
keys, the two new symbols in libzsg.so / include/zsg.h / the ctypes table, the host predicate, and the host reference of the GPU tests
(tests/wgrad_bf16_ref.py) against int64 arithmetic."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_bf16_ref as R  # noqa: E402

NEW = ("zsg_conv_wgrad_bf16", "zsg_conv_wgrad_bf16_supported")


@pytest.fixture(scope="module")
def Z():
    from zsgnet_pytorch_amd import _lib, config, mdl
    return _lib, config, mdl


def test_cfg_default_and_validation_where_the_net_is_built(Z):
    _, config, mdl = Z
    assert config.get_cfg()["wgrad_dtype"] == "fp32"
    assert mdl.get_default_net(9, config.get_cfg(resnet_arch="resnet18"))._wgrad_dtype == "fp32"
    assert mdl.get_default_net(9, config.get_cfg(resnet_arch="resnet18", wgrad_dtype="bf16"))._wgrad_dtype == "bf16"
    with pytest.raises(ValueError, match="wgrad_dtype"):
        mdl.get_default_net(9, config.get_cfg(wgrad_dtype="fp16", resnet_arch="resnet18"))


def test_wgrad_precision_returns_self_and_validates(Z):
    _, config, mdl = Z
    net = mdl.get_default_net(9, config.get_cfg(resnet_arch="resnet18"))
    assert net.wgrad_precision("bf16") is net and net._wgrad_dtype == "bf16"
    for bad in ("fp16", "BF16", "bf16_act", None, 16):
        with pytest.raises(ValueError, match="wgrad_dtype"):
            net.wgrad_precision(bad)
    assert net._wgrad_dtype == "bf16"
    assert net.wgrad_precision("fp32") is net and net._wgrad_dtype == "fp32"
    assert net.wgrad_precision() is net and net._wgrad_dtype == "fp32"


def test_precision_is_part_of_a_training_plans_identity_only(Z):
    """lowering is replaced by a recorder (no GPU here): the fp32 key is what it always was, switching drops the training plans of the
    other precision, eval plans ignore the switch"""
    _, config, mdl = Z
    net = mdl.get_default_net(9, config.get_cfg(resnet_arch="resnet18"))
    seen = []

    class FakePlan:
        _prep_pending = False

        def __init__(self, *a, **k):
            seen.append((a[1:], k))
    real, mdl._Plan = mdl._Plan, FakePlan
    try:
        net.train()
        net._plan_for(2, 128, 128, 20)
        (k32,) = list(net._plans)
        assert k32 == (2, 128, 128, 20, net._frozen_key(), net._frozen_bn_key(), net._sync_bn_key(), True)
        assert seen[-1][1]["wgrad_dtype"] == "fp32"
        net.wgrad_precision("bf16")
        net._plan_for(2, 128, 128, 20)
        (k16,) = list(net._plans)                                   # the fp32 training plan went
        assert k16 != k32 and k16[:7] == k32[:7] and k16[-1] is True and ("wgrad", "bf16") in k16
        assert seen[-1][1]["wgrad_dtype"] == "bf16"
        p16 = net._plans[k16]
        assert net._plan_for(2, 128, 128, 20) is p16                # cached
        net.shared_training(True)
        net._plan_for(2, 128, 128, 20, Q=4)
        ks = [k for k in net._plans if k != k16]
        assert len(ks) == 1 and ("shared", 4) in ks[0] and ("wgrad", "bf16") in ks[0] and seen[-1][1]["wgrad_dtype"] == "bf16"
        net._plan_for(2, 128, 128, 20, Q=6)                          # a new (B, Q) drops the old shared plan, as before
        assert [("shared", 6) in k for k in net._plans if k != k16] == [True]
        net.wgrad_precision("fp32")
        net._plan_for(2, 128, 128, 20, Q=6)
        assert list(net._plans) == [(2, 128, 128, 20, net._frozen_key(), net._frozen_bn_key(), net._sync_bn_key(), ("shared", 6), True)]
        net._plan_for(2, 128, 128, 20)
        assert k32 in net._plans and all(("wgrad", "bf16") not in k for k in net._plans)
        net.eval()
        net._plan_for(2, 128, 128, 20)
        net.wgrad_precision("bf16")
        n = len(seen)
        net._plan_for(2, 128, 128, 20)
        assert len(seen) == n and (2, 128, 128, 20, False) in net._plans, "eval plans ignore the switch"
        assert seen[-1][1].get("wgrad_dtype", "fp32") == "fp32"
    finally:
        mdl._Plan = real


def test_new_symbols_are_exported_declared_and_bound(Z):
    L = Z[0]
    hdr = open(os.path.join(ROOT, "include", "zsg.h")).read()
    so = C.CDLL(os.path.join(ROOT, "zsgnet-pytorch_amd", "libzsg.so"))
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", hdr), name
        assert name in L.SIGNATURES and hasattr(L.lib, name)
        assert getattr(so, name) is not None
    P, I32 = L.P, L.I32
    assert L.SIGNATURES["zsg_conv_wgrad_bf16"] == L.SIGNATURES["zsg_conv_wgrad"] == (I32, [L.DP, P, P, P, I32, P, L.SZ, P])
    assert L.SIGNATURES["zsg_conv_wgrad_bf16_supported"] == (I32, [L.DP])
    mk = open(os.path.join(ROOT, "zsgnet-pytorch_amd", "csrc", "Makefile")).read()
    assert "wgrad_bf16.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1)


def _desc(L):
    d = L.ConvDesc()
    d.B, d.C, d.N, d.src_ld, d.out_ld, d.wR, d.wS, d.wC, d.wt_ld, d.nseg = 2, 64, 64, 64, 64, 1, 1, 64, 64, 1
    s = d.seg[0]
    s.rows_y = s.rows_x = s.src_H = s.src_W = s.out_W = 8
    s.sy = s.sx = s.osy = s.osx = 1
    s.src_bstride = s.out_bstride = 8 * 8 * 64
    s.ty.n = s.tx.n = 1
    return d


def test_supported_answers_without_a_gpu(Z):
    """the predicate is host code: it answers on a descriptor alone; every refusal of the contract in include/zsg.h"""
    L = Z[0]
    ok = L.lib.zsg_conv_wgrad_bf16_supported
    assert ok(C.byref(_desc(L))) == 1 and ok(None) == 0
    for hint in (64 | (64 << 8) | (1 << 16), 128 | (64 << 8) | (3 << 16), 64 | (128 << 8) | (2 << 16), 128 | (128 << 8) | (255 << 16)):
        d = _desc(L)
        d.tile_hint = hint
        assert ok(C.byref(d)) == 1, hex(hint)
    bad = dict(merge_x=dict(merge_x=1), out_ld=dict(out_ld=46), bit24=dict(tile_hint=128 | (128 << 8) | (2 << 16) | (1 << 24)),
               bit25=dict(tile_hint=64 | (64 << 8) | (2 << 16) | (1 << 25)), bit27=dict(tile_hint=64 | (64 << 8) | (1 << 27)),
               bn255=dict(tile_hint=64 | (255 << 8) | (2 << 16)), tile32=dict(tile_hint=32 | (64 << 8) | (1 << 16)), c=dict(C=62))
    for what, kw in bad.items():
        d = _desc(L)
        for k, v in kw.items():
            setattr(d, k, v)
        assert ok(C.byref(d)) == 0, what
    d = _desc(L)
    d.seg[0].src_bstride = 1 << 23                                  # the fp32 entry's wide fallback
    assert ok(C.byref(d)) == 0
    d = _desc(L)
    d.seg[0].out_bstride = 1 << 23
    assert ok(C.byref(d)) == 0


def test_tuner_offers_the_bf16_entry_its_own_candidates_and_key(Z):
    import json
    from zsgnet_pytorch_amd import ops
    tj = json.load(open(ops.SHIPPED_TABLE))
    assert not any("zsg_conv_wgrad_bf16" in k for k in tj["entries"]), "no bf16 weight-gradient entries ship"
    assert tj["source_stamp"] == ops.files_stamp()
    ws = 256 << 20
    # (N, ncols, rows): head 3x3, a 1x1 of layer1, a 64-channel layer, the 45-channel output, a tiny level
    for N, ncols, rows in ((256, 2304, 5776), (256, 64, 90000), (64, 576, 90000), (45, 2304, 5776), (64, 64, 9), (2048, 512, 1600)):
        cands = ops.wgrad_bf16_cands(N, ncols, rows, ws)
        assert cands and len(cands) == len(set(cands))
        tiles = set()
        for h in cands:
            bm, bn, sp = h & 0xff, (h >> 8) & 0xff, (h >> 16) & 0xff
            assert h >> 24 == 0, "no variant bits"
            assert bm in (64, 128) and bn in (64, 128), "the entry's tiles only (no BN 255)"
            assert (bm == 64 or N > 64) and (bn == 64 or ncols > 64)
            assert 1 <= sp <= 255 and sp <= max(1, rows // 64) and sp * N * ncols * 4 <= ws
            tiles.add((bm, bn))
            d = _desc(Z[0])
            d.tile_hint = h
            assert Z[0].lib.zsg_conv_wgrad_bf16_supported(C.byref(d)) == 1, hex(h)
        assert tiles == {(bm, bn) for bm in ((64, 128) if N > 64 else (64,)) for bn in ((64, 128) if ncols > 64 else (64,))}
    # the fp32 branch's split targets: 256 .. 2048 blocks over the tile grid
    got = sorted((h >> 16) & 0xff for h in ops.wgrad_bf16_cands(256, 2304, 5776, ws) if h & 0xffff == (128 | (128 << 8)))
    assert got == sorted({max(1, min(t // 36, 5776 // 64, 255)) for t in (256, 384, 512, 768, 1024, 2048)})
    assert ops.wgrad_bf16_cands(256, 2304, 5776, 3 * 256 * 2304 * 4) and all(((h >> 16) & 0xff) <= 3 for h in ops.wgrad_bf16_cands(256, 2304, 5776, 3 * 256 * 2304 * 4))


@pytest.mark.parametrize("geo", [((5, 7), 2, 8, 12, 3, 1, 1, 1), ((9, 8), 1, 4, 5, 3, 2, 1, 1), ((12, 12), 1, 8, 6, 3, 1, 6, 6),
                                 ((6, 5), 3, 12, 7, 1, 2, 0, 1), ((4, 4), 2, 4, 4, 1, 1, 0, 1)])
def test_host_reference_agrees_with_int64_arithmetic(geo):
    """tests/wgrad_bf16_ref.py against an independent form of the same sum: the autograd weight gradient of conv2d in float64 (integer
    data: exact) and a direct int64 loop over the taps of one output channel"""
    (H, W), B, Cc, N, k, s, p, d = geo
    g = torch.Generator().manual_seed(H * 31 + W)
    Ho, Wo = R.conv_out(H, k, s, p, d), R.conv_out(W, k, s, p, d)
    src = torch.randint(-8, 9, (B, H, W, Cc), generator=g)
    dy = torch.randint(-8, 9, (B, Ho, Wo, N), generator=g)
    got = R.wgrad_ref(src, dy, k, s, p, d)
    assert got.dtype == torch.int64 and got.shape == (N, k, k, Cc)
    w = torch.zeros(N, Cc, k, k, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(src.permute(0, 3, 1, 2).double(), w, stride=s, padding=p, dilation=d)
    (gw,) = torch.autograd.grad(y, w, dy.permute(0, 3, 1, 2).double())
    assert torch.equal(got, gw.permute(0, 2, 3, 1).to(torch.int64))
    n, c = N - 1, Cc - 1                                             # one (n, c) pair by the definition, element by element
    for ty in range(k):
        for tx in range(k):
            acc = 0
            for b in range(B):
                for yy in range(Ho):
                    for xx in range(Wo):
                        sy, sx = yy * s + ty * d - p, xx * s + tx * d - p
                        if 0 <= sy < H and 0 <= sx < W:
                            acc += int(dy[b, yy, xx, n]) * int(src[b, sy, sx, c])
            assert int(got[n, ty, tx, c]) == acc
    two = R.wgrad_ref_levels([src, src], [dy, dy], k, s, p, d)
    assert torch.equal(two, 2 * got)
    x = torch.tensor([1.00390625, 1.01171875, -1.00390625, 3.0])   # ties: to even below / above
    assert torch.equal(R.bf16_round(x), torch.tensor([1.0, 1.015625, -1.0, 3.0], dtype=torch.float64))

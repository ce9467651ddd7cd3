"""enc_dtype = "bf16_fwd" without a GPU: the cfg key and its validation where the net is built, ZSGNet.encoder_precision and the wrapper's
method, the training plan keys and _Plan keywords (the fake-plan recorder of tests/test_cpu_train_bf16_head.py), the three new symbols
in libzsg.so / include/zsg.h / the ctypes table, and the host predicates on forward descriptors."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("zsg_conv_igemm_bf16_bn", "zsg_conv_igemm_bf16_bn_supported", "zsg_conv_igemm_bf16_partial_rows")


@pytest.fixture(scope="module")
def Z():
    from zsgnet_pytorch_amd import _lib, config, mdl, ops
    return _lib, config, mdl, ops


def test_cfg_default_and_validation_where_the_net_is_built(Z):
    _, config, mdl, _ = Z
    assert config.get_cfg()["enc_dtype"] == "fp32"
    assert mdl.ENC_DTYPES == ("fp32", "bf16_fwd")
    assert mdl.TRAIN_DTYPES == ("fp32", "bf16_head"), "a new switch, not a new train_dtype value"
    assert mdl.get_default_net(9, config.get_cfg(resnet_arch="resnet18"))._enc_dtype == "fp32"
    assert mdl.get_default_net(9, config.get_cfg(resnet_arch="resnet18", enc_dtype="bf16_fwd"))._enc_dtype == "bf16_fwd"
    for bad in ("bf16", "fp16", "bf16_head"):
        with pytest.raises(ValueError, match="enc_dtype"):
            mdl.get_default_net(9, config.get_cfg(enc_dtype=bad, resnet_arch="resnet18"))
    # independent of the other three switches
    net = mdl.get_default_net(9, config.get_cfg(resnet_arch="resnet18", enc_dtype="bf16_fwd", train_dtype="bf16_head", wgrad_dtype="bf16",
                                                eval_dtype="bf16_act"))
    assert (net._enc_dtype, net._train_dtype, net._wgrad_dtype, net._eval_dtype) == ("bf16_fwd", "bf16_head", "bf16", "bf16_act")
    net = mdl.get_default_net(9, config.get_cfg(resnet_arch="resnet18", enc_dtype="bf16_fwd"))
    assert (net._train_dtype, net._wgrad_dtype, net._eval_dtype) == ("fp32", "fp32", "fp32")


def test_encoder_precision_returns_self_and_validates(Z):
    _, config, mdl, _ = Z
    net = mdl.get_default_net(9, config.get_cfg(resnet_arch="resnet18"))
    assert net.encoder_precision("bf16_fwd") is net and net._enc_dtype == "bf16_fwd"
    for bad in ("bf16", "fp16", None, "BF16_FWD", 16):
        with pytest.raises(ValueError, match="enc_dtype"):
            net.encoder_precision(bad)
    assert net._enc_dtype == "bf16_fwd"
    assert net._train_dtype == "fp32" and net._wgrad_dtype == "fp32" and net._eval_dtype == "fp32"
    with pytest.raises(ValueError, match="train_dtype"):
        net.train_precision("bf16")                                   # (still free for a whole-network version)
    assert net.encoder_precision("fp32") is net and net._enc_dtype == "fp32"
    assert net.encoder_precision() is net and net._enc_dtype == "fp32"


def test_wrapper_forwards_encoder_precision_and_keys_its_tuner_exchange_on_it(Z, monkeypatch):
    _, config, mdl, _ = Z
    from zsgnet_pytorch_amd import dist as zdist
    net = mdl.get_default_net(9, config.get_cfg(resnet_arch="resnet18"))
    lowered = []
    monkeypatch.setattr(net, "_plan_for", lambda *a, **k: lowered.append(a))
    monkeypatch.setattr(zdist, "get_rank", lambda *a, **k: 0)
    monkeypatch.setattr(zdist.dist, "broadcast_object_list", lambda *a, **k: None)
    ddp = object.__new__(zdist.DistributedDataParallel)
    torch.nn.Module.__init__(ddp)
    ddp.module, ddp.group, ddp._tuned = net, None, set()
    inp = dict(img=torch.zeros(2, 3, 128, 128), qvec=torch.zeros(2, 20, 300), qlens=torch.ones(2))
    net.train()
    ddp._sync_tuning(inp)
    (k32,) = ddp._tuned
    assert not any(isinstance(e, tuple) and e[:1] == ("enc",) for e in k32)
    assert ddp.encoder_precision("bf16_fwd") is ddp and net._enc_dtype == "bf16_fwd"
    ddp._sync_tuning(inp)
    (k16,) = ddp._tuned - {k32}
    assert k16 == k32 + (("enc", "bf16_fwd"),), "the same geometry under the new precision is exchanged again"
    net.wgrad_precision("bf16").train_precision("bf16_head")
    ddp._sync_tuning(inp)
    (kb,) = ddp._tuned - {k32, k16}
    assert kb == k32 + (("wgrad", "bf16"), ("train", "bf16_head"), ("enc", "bf16_fwd"))
    net.eval()
    ddp._sync_tuning(inp)
    (ke,) = ddp._tuned - {k32, k16, kb}
    assert not any(isinstance(e, tuple) and e[:1] in (("train",), ("wgrad",), ("enc",)) for e in ke), "eval plans ignore the switch"
    with pytest.raises(ValueError, match="enc_dtype"):
        ddp.encoder_precision("bf16")


def _record(mdl):
    seen = []

    class FakePlan:
        _prep_pending = False

        def __init__(self, *a, **k):
            seen.append((a[1:], k))
    return seen, FakePlan


def test_precision_is_part_of_a_training_plans_identity_only(Z):
    """lowering is replaced by a recorder (no GPU here): with the default, keys and _Plan keywords are those of a net that never saw the
    key; the training key carries ("enc", "bf16_fwd") only when on; switching drops the training plans of the other value; eval plans
    neither see the switch nor receive the keyword"""
    _, config, mdl, _ = Z
    cfg_plain = config.get_cfg(resnet_arch="resnet18")
    del cfg_plain["enc_dtype"]                                        # a configuration from before the key existed
    never = mdl.get_default_net(9, cfg_plain)
    net = mdl.get_default_net(9, config.get_cfg(resnet_arch="resnet18", enc_dtype="fp32"))
    seen, Fake = _record(mdl)
    real, mdl._Plan = mdl._Plan, Fake
    try:
        never.train()
        never._plan_for(2, 128, 128, 20)
        ref_args, ref_kw = seen[-1]
        net.train()
        net._plan_for(2, 128, 128, 20)
        (k32,) = list(net._plans)
        assert k32 == (2, 128, 128, 20, net._frozen_key(), net._frozen_bn_key(), net._sync_bn_key(), True) and list(never._plans) == [k32]
        assert seen[-1] == (ref_args, ref_kw) and "enc_dtype" not in seen[-1][1]
        assert set(ref_kw) == {"frozen", "frozen_bn", "sync_bn", "wgrad_dtype", "train_dtype"}, "the parent's keyword set"
        net.encoder_precision("bf16_fwd")
        net._plan_for(2, 128, 128, 20)
        (k16,) = list(net._plans)                                    # the fp32 training plan went
        assert k16 == k32[:7] + (("enc", "bf16_fwd"), True)
        assert seen[-1][1]["enc_dtype"] == "bf16_fwd" and seen[-1][1]["train_dtype"] == "fp32" and seen[-1][1]["wgrad_dtype"] == "fp32"
        assert net._key_enc(k16) == "bf16_fwd" and net._key_enc(k32) == "fp32" and net._key_train(k16) == "fp32" and net._key_wgrad(k16) == "fp32"
        assert net._plan_for(2, 128, 128, 20) is net._plans[k16]     # cached
        net.wgrad_precision("bf16").train_precision("bf16_head")     # the switches combine; each is its own key field
        net._plan_for(2, 128, 128, 20)
        (kb,) = list(net._plans)
        assert kb == k32[:7] + (("wgrad", "bf16"), ("train", "bf16_head"), ("enc", "bf16_fwd"), True)
        assert [seen[-1][1][k] for k in ("wgrad_dtype", "train_dtype", "enc_dtype")] == ["bf16", "bf16_head", "bf16_fwd"]
        net.wgrad_precision("fp32").train_precision("fp32")
        net._plan_for(2, 128, 128, 20)
        assert list(net._plans) == [k16]
        net.shared_training(True)
        net._plan_for(2, 128, 128, 20, Q=4)
        ks = [k for k in net._plans if k != k16]
        assert len(ks) == 1 and ("shared", 4) in ks[0] and ("enc", "bf16_fwd") in ks[0] and seen[-1][1]["enc_dtype"] == "bf16_fwd"
        net.encoder_precision("fp32")
        net._plan_for(2, 128, 128, 20, Q=4)
        assert list(net._plans) == [(2, 128, 128, 20, net._frozen_key(), net._frozen_bn_key(), net._sync_bn_key(), ("shared", 4), True)]
        assert "enc_dtype" not in seen[-1][1]
        net._plan_for(2, 128, 128, 20)
        assert k32 in net._plans and all(("enc", "bf16_fwd") not in k for k in net._plans) and "enc_dtype" not in seen[-1][1]
        net.eval()
        net._plan_for(2, 128, 128, 20)
        net.encoder_precision("bf16_fwd")
        n = len(seen)
        net._plan_for(2, 128, 128, 20)
        assert len(seen) == n and (2, 128, 128, 20, False) in net._plans, "eval plans ignore the switch"
        assert "enc_dtype" not in seen[-1][1]
        net.eval_precision("bf16")
        net._plan_for(2, 128, 128, 20)
        assert (2, 128, 128, 20, "bf16", False) in net._plans and "enc_dtype" not in seen[-1][1]
        net._plan_for(2, 128, 128, 20, Q=4)
        assert "enc_dtype" not in seen[-1][1]
    finally:
        mdl._Plan = real


def test_plan_accepts_the_keyword_and_covers_resnet_only(Z):
    import inspect
    mdl = Z[2]
    sig = inspect.signature(mdl._Plan.__init__)
    assert sig.parameters["enc_dtype"].default == "fp32"
    assert mdl.BF16_ENC_PREFIX == "backbone.encoder." and not any(p.startswith(mdl.BF16_ENC_PREFIX) for p in mdl.BF16_HEAD_PREFIXES)


def test_new_symbols_are_exported_declared_and_bound(Z):
    L = Z[0]
    hdr = open(os.path.join(ROOT, "include", "zsg.h")).read()
    so = C.CDLL(os.path.join(ROOT, "zsgnet-pytorch_amd", "libzsg.so"))
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", hdr), name
        assert name in L.SIGNATURES and hasattr(L.lib, name)
        assert getattr(so, name) is not None
    P, I32 = L.P, L.I32
    assert L.SIGNATURES["zsg_conv_igemm_bf16_bn"] == (I32, [L.DP, P, P, P, P, P])        # (d, src, wt_packed, out, bn_partials, stream)
    assert L.SIGNATURES["zsg_conv_igemm_bf16_bn_supported"] == (I32, [L.DP])
    assert L.SIGNATURES["zsg_conv_igemm_bf16_partial_rows"] == (I32, [L.DP])


def _fwd(ops, H, W, B, Cc, Nn, k, s, p, **kw):
    Ho, Wo = ops.conv_out(H, k, s, p), ops.conv_out(W, k, s, p)
    x = ops.TView(torch.zeros(1), B, Cc, Cc, [ops.Level(0, H, W, H * W * Cc)])
    o = ops.TView(torch.zeros(1), B, Nn, Nn, [ops.Level(0, Ho, Wo, Ho * Wo * Nn)])
    d = ops.fwd_desc(x, o, Cc, Nn, k, s, p, 1, wC=Cc)
    for k_, v in kw.items():
        setattr(d, k_, v)
    return d


def test_predicates_answer_without_a_gpu(Z):
    """host code: the encoder's convolution shapes are accepted and the partial rows are sum ceil(rows / BM) for the hinted tile; what
    zsg_conv_igemm_bf16 refuses, ReLU, N % 4 != 0 and an output layout off the 16-byte epilogue are refused with -1 rows"""
    L, _, _, ops = Z
    ok, rows_of = L.lib.zsg_conv_igemm_bf16_bn_supported, L.lib.zsg_conv_igemm_bf16_partial_rows
    assert ok(None) == 0 and rows_of(None) == -1
    shapes = [(75, 75, 16, 64, 64, 1, 1, 0), (75, 75, 16, 64, 64, 3, 1, 1), (75, 75, 16, 256, 128, 1, 1, 0), (75, 75, 16, 128, 128, 3, 2, 1),
              (75, 75, 16, 256, 512, 1, 2, 0), (9, 9, 2, 64, 256, 1, 1, 0)]
    for sh in shapes:
        d = _fwd(ops, *sh)
        n = sh[2] * ops.conv_out(sh[0], sh[5], sh[6], sh[7]) * ops.conv_out(sh[1], sh[5], sh[6], sh[7])
        assert ok(C.byref(d)) == 1, sh
        assert rows_of(C.byref(d)) in ((n + 63) // 64, (n + 127) // 128), sh        # hint 0: whichever tile the heuristic picks
        for bm, bn in ((64, 64), (128, 64), (128, 128)):
            d.tile_hint = ops.tile_hint(bm, bn, 1)
            assert ok(C.byref(d)) == 1 and rows_of(C.byref(d)) == (n + bm - 1) // bm, (sh, bm, bn)
    bad = dict(relu=dict(relu=1), n4=dict(N=62), merge_x=dict(merge_x=1), split=dict(tile_hint=ops.tile_hint(64, 64, 2)), epi=dict(epi_flags=1),
               streamk=dict(tile_hint=ops.tile_hint(64, 64, 1) | (1 << 28)), tile=dict(tile_hint=ops.tile_hint(32, 64, 1)), out_ld=dict(out_ld=66))
    for what, kw in bad.items():
        d = _fwd(ops, 9, 9, 2, 64, 64, 1, 1, 0, **kw)
        assert ok(C.byref(d)) == 0 and rows_of(C.byref(d)) == -1, what

"""train_dtype = "bf16_head" without a GPU: the cfg key and its validation where the net is built, ZSGNet.train_precision, the training plan
keys (the fake-plan recorder of tests/test_cpu_wgrad_bf16.py), the two new symbols in libzsg.so / include/zsg.h / the ctypes table, and
the host predicate zsg_conv_igemm_bf16_m_supported on data-gradient descriptors."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("zsg_conv_igemm_bf16_m", "zsg_conv_igemm_bf16_m_supported")


@pytest.fixture(scope="module")
def Z():
    from zsgnet_pytorch_amd import _lib, config, mdl, ops
    return _lib, config, mdl, ops


def test_cfg_default_and_validation_where_the_net_is_built(Z):
    _, config, mdl, _ = Z
    assert config.get_cfg()["train_dtype"] == "fp32"
    assert mdl.TRAIN_DTYPES == ("fp32", "bf16_head")
    assert mdl.get_default_net(9, config.get_cfg(resnet_arch="resnet18"))._train_dtype == "fp32"
    assert mdl.get_default_net(9, config.get_cfg(resnet_arch="resnet18", train_dtype="bf16_head"))._train_dtype == "bf16_head"
    for bad in ("bf16", "fp16"):                                     # ("bf16" is kept free for a whole-network version)
        with pytest.raises(ValueError, match="train_dtype"):
            mdl.get_default_net(9, config.get_cfg(train_dtype=bad, resnet_arch="resnet18"))
    # independent of the other two switches
    net = mdl.get_default_net(9, config.get_cfg(resnet_arch="resnet18", train_dtype="bf16_head", wgrad_dtype="bf16", eval_dtype="bf16_act"))
    assert (net._train_dtype, net._wgrad_dtype, net._eval_dtype) == ("bf16_head", "bf16", "bf16_act")


def test_train_precision_returns_self_and_validates(Z):
    _, config, mdl, _ = Z
    net = mdl.get_default_net(9, config.get_cfg(resnet_arch="resnet18"))
    assert net.train_precision("bf16_head") is net and net._train_dtype == "bf16_head"
    for bad in ("bf16", "fp16", None, "BF16_HEAD", 16):
        with pytest.raises(ValueError, match="train_dtype"):
            net.train_precision(bad)
    assert net._train_dtype == "bf16_head"
    assert net._wgrad_dtype == "fp32" and net._eval_dtype == "fp32"
    assert net.train_precision("fp32") is net and net._train_dtype == "fp32"
    assert net.train_precision() is net and net._train_dtype == "fp32"


def test_wrapper_forwards_train_precision_and_keys_its_tuner_exchange_on_it(Z, monkeypatch):
    """the wrapper without a process group (its collectives stubbed, lowering replaced by a recorder): train_precision forwards to the
    network and returns the wrapper; the key under which the tuner entries are exchanged gains ("train", dtype) for a training
    network with the switch on — and only then"""
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
    assert not any(isinstance(e, tuple) and e[:1] == ("train",) for e in k32)
    assert ddp.train_precision("bf16_head") is ddp and net._train_dtype == "bf16_head"
    ddp._sync_tuning(inp)
    (k16,) = ddp._tuned - {k32}
    assert k16 == k32 + (("train", "bf16_head"),), "the same geometry under the new precision is exchanged again"
    net.wgrad_precision("bf16")
    ddp._sync_tuning(inp)
    (kb,) = ddp._tuned - {k32, k16}
    assert kb == k32 + (("wgrad", "bf16"), ("train", "bf16_head"))
    n = len(lowered)
    ddp._sync_tuning(inp)
    assert len(ddp._tuned) == 3 and len(lowered) == n, "a key already exchanged is not exchanged again"
    net.eval()
    ddp._sync_tuning(inp)
    (ke,) = ddp._tuned - {k32, k16, kb}
    assert not any(isinstance(e, tuple) and e[:1] in (("train",), ("wgrad",)) for e in ke), "eval plans ignore the switch"
    with pytest.raises(ValueError, match="train_dtype"):
        ddp.train_precision("bf16")


def test_precision_is_part_of_a_training_plans_identity_only(Z):
    """lowering is replaced by a recorder (no GPU here): the fp32 key is what it always was, the training key carries the switch next to
    wgrad's, switching drops the training plans of the other precision, eval plans ignore the switch"""
    _, config, mdl, _ = Z
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
        assert seen[-1][1]["train_dtype"] == "fp32" and seen[-1][1]["wgrad_dtype"] == "fp32"
        net.train_precision("bf16_head")
        net._plan_for(2, 128, 128, 20)
        (k16,) = list(net._plans)                                   # the fp32 training plan went
        assert k16 == k32[:7] + (("train", "bf16_head"), True)
        assert seen[-1][1]["train_dtype"] == "bf16_head" and seen[-1][1]["wgrad_dtype"] == "fp32"
        assert net._key_train(k16) == "bf16_head" and net._key_train(k32) == "fp32" and net._key_wgrad(k16) == "fp32"
        p16 = net._plans[k16]
        assert net._plan_for(2, 128, 128, 20) is p16                # cached
        net.wgrad_precision("bf16")                                  # the two switches combine; each is its own key field
        net._plan_for(2, 128, 128, 20)
        (kb,) = list(net._plans)
        assert kb == k32[:7] + (("wgrad", "bf16"), ("train", "bf16_head"), True)
        assert seen[-1][1]["train_dtype"] == "bf16_head" and seen[-1][1]["wgrad_dtype"] == "bf16"
        net.wgrad_precision("fp32")
        net._plan_for(2, 128, 128, 20)
        assert list(net._plans) == [k16]
        net.shared_training(True)
        net._plan_for(2, 128, 128, 20, Q=4)
        ks = [k for k in net._plans if k != k16]
        assert len(ks) == 1 and ("shared", 4) in ks[0] and ("train", "bf16_head") in ks[0] and seen[-1][1]["train_dtype"] == "bf16_head"
        net.train_precision("fp32")
        net._plan_for(2, 128, 128, 20, Q=4)
        assert list(net._plans) == [(2, 128, 128, 20, net._frozen_key(), net._frozen_bn_key(), net._sync_bn_key(), ("shared", 4), True)]
        net._plan_for(2, 128, 128, 20)
        assert k32 in net._plans and all(("train", "bf16_head") not in k for k in net._plans)
        net.eval()
        net._plan_for(2, 128, 128, 20)
        net.train_precision("bf16_head")
        n = len(seen)
        net._plan_for(2, 128, 128, 20)
        assert len(seen) == n and (2, 128, 128, 20, False) in net._plans, "eval plans ignore the switch"
        assert seen[-1][1].get("train_dtype", "fp32") == "fp32"
        net.eval_precision("bf16")
        net._plan_for(2, 128, 128, 20)
        assert (2, 128, 128, 20, "bf16", False) in net._plans and "train_dtype" not in seen[-1][1]
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
    # zsg_conv_igemm_bf16's arguments with mask_src in front of the stream
    assert L.SIGNATURES["zsg_conv_igemm_bf16_m"] == (I32, [L.DP, P, P, P, P, P, P, P])
    assert len(L.SIGNATURES["zsg_conv_igemm_bf16_m"][1]) == len(L.SIGNATURES["zsg_conv_igemm_bf16"][1]) + 1
    assert L.SIGNATURES["zsg_conv_igemm_bf16_m_supported"] == (I32, [L.DP])


def _dgrad(ops, levels_dx, B, cred, n, k, stride, pad):
    """ops.dgrad_desc for dy [B, ., ., cred] -> dx [B, H, W, n] over packed levels"""
    def pack(sizes, ld):
        lv, off = [], 0
        for (h, w) in sizes:
            lv.append(ops.Level(off, h, w, h * w * ld))
            off += B * h * w * ld
        return lv, off
    dy_sizes = [(ops.conv_out(h, k, stride, pad), ops.conv_out(w, k, stride, pad)) for h, w in levels_dx]
    lx, nx = pack(levels_dx, n)
    ly, ny = pack(dy_sizes, cred)
    dy = ops.TView(torch.zeros(1), B, cred, cred, ly)
    dx = ops.TView(torch.zeros(1), B, n, n, lx)
    return ops.dgrad_desc(dy, dx, cred, n, k, stride, pad, 1)


def test_supported_answers_without_a_gpu(Z):
    """the predicate is host code: it accepts the data-gradient descriptors of the shared head and a stride-2 one, and refuses what
    zsg_conv_igemm_bf16 refuses (one check list)"""
    L, _, _, ops = Z
    ok, ok0 = L.lib.zsg_conv_igemm_bf16_m_supported, L.lib.zsg_conv_igemm_bf16_supported
    assert ok(None) == 0
    head = lambda: _dgrad(ops, [(38, 38), (19, 19), (10, 10), (5, 5), (3, 3), (1, 1)], 16, 256, 256, 3, 1, 1)
    last = lambda: _dgrad(ops, [(10, 10), (5, 5), (3, 3)], 2, 48, 256, 3, 1, 1)            # the 45 -> 48 padded output gradient
    s2 = lambda: _dgrad(ops, [(5, 5)], 2, 256, 256, 3, 2, 1)
    assert s2().nseg == 4 and not s2().zero_fill
    for mk in (head, last, s2):
        d = mk()
        assert ok(C.byref(d)) == 1 and ok0(C.byref(d)) == 1
        for hint in (ops.tile_hint(64, 64, 1), ops.tile_hint(128, 64, 1), ops.tile_hint(128, 128, 1), ops.tile_hint(64, 64, 0)):
            d = mk()
            d.tile_hint = hint
            assert ok(C.byref(d)) == 1, hex(hint)
        bad = dict(merge_x=dict(merge_x=1), split=dict(tile_hint=ops.tile_hint(64, 64, 2)), split8=dict(tile_hint=ops.tile_hint(128, 64, 8)),
                   epi=dict(epi_flags=1), streamk=dict(tile_hint=ops.tile_hint(64, 64, 1) | (1 << 28)), w8=dict(tile_hint=ops.tile_hint(64, 64, 1, 1)),
                   tile=dict(tile_hint=ops.tile_hint(32, 64, 1)))
        for what, kw in bad.items():
            d = mk()
            for k_, v in kw.items():
                setattr(d, k_, v)
            assert ok(C.byref(d)) == 0 and ok0(C.byref(d)) == 0, what


def test_shipped_table_has_no_entries_for_the_new_launches(Z):
    """the shipped table moved to the new source stamp and gained nothing (holds without the feature's lowering: a check of the table,
    no part of the feature's coverage)"""
    import json
    ops = Z[3]
    tj = json.load(open(ops.SHIPPED_TABLE))
    assert not any("zsg_conv_igemm_bf16_m" in k for k in tj["entries"])
    assert tj["source_stamp"] == ops.files_stamp()

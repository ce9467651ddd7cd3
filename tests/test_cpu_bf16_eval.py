"""eval_dtype = "bf16" without a GPU: the cfg key, its validation where the net is built, ZSGNet.eval_precision, the plan-cache keys,
the three new symbols in include/zsg.h and the ctypes table, tools/eval_speed.py --dtype."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("zsg_conv_igemm_bf16", "zsg_conv_igemm_bf16_supported", "zsg_pack_w_bf16_batched")


@pytest.fixture(scope="module")
def Z():
    from zsgnet_pytorch_amd import _lib, config, mdl
    return _lib, config, mdl


def test_cfg_key_and_validation_where_the_net_is_built(Z):
    _, config, mdl = Z
    assert config.get_cfg()["eval_dtype"] == "fp32"
    cfg = config.get_cfg(eval_dtype="bf16", resnet_arch="resnet18")
    assert cfg["eval_dtype"] == "bf16"
    net = mdl.get_default_net(9, cfg)
    assert net._eval_dtype == "bf16"
    assert mdl.get_default_net(9, config.get_cfg(resnet_arch="resnet18"))._eval_dtype == "fp32"
    with pytest.raises(ValueError, match="eval_dtype"):
        mdl.get_default_net(9, config.get_cfg(eval_dtype="fp16", resnet_arch="resnet18"))


def test_eval_precision_returns_self_validates_and_keys_the_eval_plans_only(Z):
    _, config, mdl = Z
    net = mdl.get_default_net(9, config.get_cfg(resnet_arch="resnet18"))
    assert net._eval_key(2, 128, 128, 20) == (2, 128, 128, 20, False)                       # the default keeps the key it always had
    assert net._eval_key(2, 128, 128, 20, Q=4) == (2, 4, 128, 128, 20, "shared", False)
    assert net.eval_precision("bf16") is net and net._eval_dtype == "bf16"
    assert net._eval_key(2, 128, 128, 20) == (2, 128, 128, 20, "bf16", False)
    assert net._eval_key(2, 128, 128, 20, Q=4) == (2, 4, 128, 128, 20, "shared", "bf16", False)
    for bad in ("fp16", "BF16", None, 16):
        with pytest.raises(ValueError, match="eval_dtype"):
            net.eval_precision(bad)
    assert net._eval_dtype == "bf16"
    # the train-mode plan key does not know the dtype: lowering is replaced by a recorder (no GPU here)
    seen = []

    class FakePlan:
        _prep_pending = False

        def __init__(self, *a, **k):
            seen.append((a[1:], k))
    real, mdl._Plan = mdl._Plan, FakePlan
    try:
        net.train()
        net._plan_for(2, 128, 128, 20)
        key_bf = list(net._plans)
        net.eval_precision("fp32")
        net._plan_for(2, 128, 128, 20)
        assert list(net._plans) == key_bf and len(key_bf) == 1 and "bf16" not in key_bf[0] and key_bf[0][-1] is True
        assert "dtype" not in seen[0][1], "a training plan is lowered without a dtype"
        net.eval()
        net._plan_for(2, 128, 128, 20)
        net.eval_precision("bf16")
        net._plan_for(2, 128, 128, 20)
        net._plan_for(2, 128, 128, 20)
        assert [k for k in net._plans if not k[-1]] == [(2, 128, 128, 20, False), (2, 128, 128, 20, "bf16", False)]
        assert [k.get("dtype") for _, k in seen[1:]] == ["fp32", "bf16"]
        # shared eval plans of both dtypes share the one LRU bound
        for q in range(3, 3 + mdl.SHARED_PLANS_MAX):
            net._plan_for(2, 128, 128, 20, Q=q)
            net.eval_precision("fp32" if q % 2 else "bf16")
        assert len([k for k in net._plans if k[5:6] == ("shared",)]) == mdl.SHARED_PLANS_MAX
        net._plan_for(2, 128, 128, 20, Q=99)
        assert len([k for k in net._plans if k[5:6] == ("shared",)]) == mdl.SHARED_PLANS_MAX
    finally:
        mdl._Plan = real
    with pytest.raises(TypeError, match="eval_precision"):
        net.double()


def test_new_symbols_are_declared_and_bound(Z):
    L = Z[0]
    hdr = open(os.path.join(ROOT, "include", "zsg.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", hdr), name
        assert name in L.SIGNATURES and hasattr(L.lib, name)
    P, I32 = L.P, L.I32
    assert L.SIGNATURES["zsg_conv_igemm_bf16"] == (I32, [L.DP, P, P, P, P, P, P])
    assert L.SIGNATURES["zsg_conv_igemm_bf16_supported"] == (I32, [L.DP])
    assert L.SIGNATURES["zsg_pack_w_bf16_batched"] == (I32, [P, I32, I32, P])
    mk = open(os.path.join(ROOT, "zsgnet-pytorch_amd", "csrc", "Makefile")).read()
    assert "igemm_bf16.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1)


def test_supported_answers_without_a_gpu(Z):
    """the predicate is host code: it answers on a descriptor alone"""
    import ctypes as C
    L = Z[0]
    d = L.ConvDesc()
    d.B, d.C, d.N, d.src_ld, d.out_ld, d.wR, d.wS, d.nseg = 2, 64, 64, 64, 64, 1, 1, 1
    s = d.seg[0]
    s.rows_y = s.rows_x = s.src_H = s.src_W = s.out_W = 8
    s.sy = s.sx = s.osy = s.osx = 1
    s.src_bstride = s.out_bstride = 8 * 8 * 64
    s.ty.n = s.tx.n = 1
    assert L.lib.zsg_conv_igemm_bf16_supported(C.byref(d)) == 1
    d.merge_x = 1
    assert L.lib.zsg_conv_igemm_bf16_supported(C.byref(d)) == 0
    d.merge_x, d.tile_hint = 0, 64 | (64 << 8) | (2 << 16)
    assert L.lib.zsg_conv_igemm_bf16_supported(C.byref(d)) == 0
    d.tile_hint = 128 | (128 << 8)
    assert L.lib.zsg_conv_igemm_bf16_supported(C.byref(d)) == 1
    assert L.lib.zsg_conv_igemm_bf16_supported(None) == 0


def test_autotune_key_carries_the_dtype(Z):
    """ZSG_AUTOTUNE=0 / no GPU: the tuner returns the heuristic; with a GPU the key's dtype field is 'bf16' for the bf16 entry and stays
    'fp32' for every other entry (the shipped table's keys are unchanged)"""
    import json
    from zsgnet_pytorch_amd import ops
    tj = json.load(open(ops.SHIPPED_TABLE))
    assert tj["entries"] and not any("'bf16'" in k for k in tj["entries"]), "no bf16 entries ship: the first bf16 eval forward tunes"
    assert all("'fp32'" in k for k in tj["entries"] if k.startswith("('igemm'"))
    assert tj["source_stamp"] == ops.files_stamp(), "the shipped table must carry the stamp of the sources it ships with"
    src = open(os.path.join(ROOT, "zsgnet-pytorch_amd", "ops.py")).read()
    assert '"bf16" if bf16 else "fp32"' in src


def test_eval_speed_parses_dtype():
    tool = os.path.join(ROOT, "tools", "eval_speed.py")
    r = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--dtype" in r.stdout and "bf16" in r.stdout
    r = subprocess.run([sys.executable, tool, "--dtype", "fp16"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "invalid choice" in r.stderr

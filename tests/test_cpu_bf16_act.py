"""eval_dtype = "bf16_act" without a GPU: the cfg key and its validation, ZSGNet.eval_precision and the plan-cache keys, the new symbols in
include/zsg.h / the ctypes table / the Makefile, the host-side predicate zsg_conv_igemm_bf16_io_supported, tools/eval_speed.py --dtype."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("zsg_conv_igemm_bf16_io", "zsg_conv_igemm_bf16_io_supported", "zsg_maxpool_fwd_bf16", "zsg_upsample_add_fwd_bf16", "zsg_relu_fwd_bf16",
       "zsg_avgpool_fwd_bf16", "zsg_head_shared_conv0_bf16", "zsg_cast_f32_bf16", "zsg_cast_bf16_f32")
SRC, OUT, ADD = 1, 2, 4


@pytest.fixture(scope="module")
def Z():
    from zsgnet_pytorch_amd import _lib, config, mdl
    return _lib, config, mdl


def test_cfg_key_and_validation_where_the_net_is_built(Z):
    _, config, mdl = Z
    cfg = config.get_cfg(eval_dtype="bf16_act", resnet_arch="resnet18")
    assert cfg["eval_dtype"] == "bf16_act"
    assert mdl.get_default_net(9, cfg)._eval_dtype == "bf16_act"
    assert "bf16_act" in mdl.EVAL_DTYPES
    with pytest.raises(ValueError, match="eval_dtype"):
        mdl.get_default_net(9, config.get_cfg(eval_dtype="fp16", resnet_arch="resnet18"))


def test_eval_precision_and_the_plan_keys(Z):
    _, config, mdl = Z
    net = mdl.get_default_net(9, config.get_cfg(resnet_arch="resnet18"))
    assert net.eval_precision("bf16_act") is net and net._eval_dtype == "bf16_act"
    assert net._eval_key(2, 128, 128, 20) == (2, 128, 128, 20, "bf16_act", False)
    assert net._eval_key(2, 128, 128, 20, Q=4) == (2, 4, 128, 128, 20, "shared", "bf16_act", False)
    for bad in ("fp16", "bf16-act", "BF16_ACT", None):
        with pytest.raises(ValueError, match="eval_dtype"):
            net.eval_precision(bad)
    assert net._eval_dtype == "bf16_act"
    assert net.eval_precision("bf16")._eval_key(2, 128, 128, 20) == (2, 128, 128, 20, "bf16", False)
    assert net.eval_precision("fp32")._eval_key(2, 128, 128, 20) == (2, 128, 128, 20, False)
    # lowering replaced by a recorder (no GPU here): the plan is built with the dtype, a training plan without one; shared plans of all three
    # dtypes share the one LRU bound
    seen = []

    class FakePlan:
        _prep_pending = False

        def __init__(self, *a, **k):
            seen.append(k)
    real, mdl._Plan = mdl._Plan, FakePlan
    try:
        net.eval()
        for dt in ("fp32", "bf16", "bf16_act", "bf16_act"):
            net.eval_precision(dt)._plan_for(2, 128, 128, 20)
        assert [k.get("dtype") for k in seen] == ["fp32", "bf16", "bf16_act"]
        assert [k for k in net._plans] == [(2, 128, 128, 20, False), (2, 128, 128, 20, "bf16", False), (2, 128, 128, 20, "bf16_act", False)]
        net.train()
        net._plan_for(2, 128, 128, 20)
        assert "dtype" not in seen[-1] and not any("bf16_act" in k for k in net._plans if k[-1])
        net.eval()
        for q in range(3, 4 + mdl.SHARED_PLANS_MAX):
            net.eval_precision(("fp32", "bf16", "bf16_act")[q % 3])._plan_for(2, 128, 128, 20, Q=q)
        assert len([k for k in net._plans if k[5:6] == ("shared",)]) == mdl.SHARED_PLANS_MAX
    finally:
        mdl._Plan = real


def test_new_symbols_are_declared_and_bound(Z):
    L = Z[0]
    hdr = open(os.path.join(ROOT, "include", "zsg.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", hdr), name
        assert name in L.SIGNATURES and hasattr(L.lib, name)
    P, I32 = L.P, L.I32
    assert L.SIGNATURES["zsg_conv_igemm_bf16_io"] == (I32, [L.DP, P, P, P, P, P, I32, P])
    assert L.SIGNATURES["zsg_conv_igemm_bf16_io_supported"] == (I32, [L.DP, I32])
    assert L.SIGNATURES["zsg_conv_igemm_bf16"] == (I32, [L.DP, P, P, P, P, P, P]), "the existing entry keeps its signature"
    for flag, v in (("ZSG_IO_SRC_BF16", SRC), ("ZSG_IO_OUT_BF16", OUT), ("ZSG_IO_ADD_BF16", ADD)):
        assert re.search(r"#define\s+" + flag + r"\s+" + str(v) + r"\b", hdr), flag
    mk = open(os.path.join(ROOT, "zsgnet-pytorch_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1)
    assert "bf16_act.hip" in srcs and "igemm_bf16.hip" in srcs


def desc(L, C_=64, N=64, src_ld=None, out_ld=None, hw=8, k=1):
    d = L.ConvDesc()
    d.B, d.C, d.N, d.src_ld, d.out_ld, d.wR, d.wS, d.nseg = 2, C_, N, src_ld or C_, out_ld or N, k, k, 1
    s = d.seg[0]
    s.rows_y = s.rows_x = s.src_H = s.src_W = s.out_W = hw
    s.sy = s.sx = s.osy = s.osx = 1
    s.src_bstride, s.out_bstride = hw * hw * d.src_ld, hw * hw * d.out_ld
    s.ty.n = s.tx.n = k
    s.ty.wstep = s.tx.wstep = s.ty.dstep = s.tx.dstep = 1
    s.ty.d0 = s.tx.d0 = -(k // 2)
    return d


def test_io_supported_answers_without_a_gpu(Z):
    """the predicate is host code: it answers on a descriptor and a flag word alone"""
    L = Z[0]
    ok = L.lib.zsg_conv_igemm_bf16_io_supported
    d = desc(L)
    for io in range(8):                      # every combination of SRC | OUT | ADD on an aligned descriptor
        assert ok(C.byref(d), io) == 1, io
    # ADD_BF16 only says how add_src is stored; whether there IS one is the entry's argument (the entry refuses the flag without it)
    assert ok(C.byref(d), ADD) == 1 and ok(C.byref(d), SRC | OUT | ADD) == 1
    for io in (-1, 8, 16, 255):
        assert ok(C.byref(d), io) == 0, io
    assert ok(None, 0) == 0 and ok(None, SRC | OUT) == 0
    # the refusals of zsg_conv_igemm_bf16 hold for every flag word
    for io in (0, SRC | OUT, SRC | OUT | ADD):
        d = desc(L)
        d.merge_x = 1
        assert ok(C.byref(d), io) == 0
        d.merge_x, d.tile_hint = 0, 64 | (64 << 8) | (2 << 16)          # split-K
        assert ok(C.byref(d), io) == 0
        d.tile_hint = 64 | (64 << 8) | (1 << 28)                       # stream-K
        assert ok(C.byref(d), io) == 0
        d.tile_hint = 64 | (64 << 8) | (1 << 24)                       # variant bits
        assert ok(C.byref(d), io) == 0
        d.tile_hint, d.epi_flags = 0, 1
        assert ok(C.byref(d), io) == 0
        d.epi_flags, d.tile_hint = 0, 128 | (128 << 8)
        assert ok(C.byref(d), io) == 1
    # rows that are only 8-byte aligned in bf16 (C = 36, src_ld = 36) are served by the two-halves loader; src_ld = 34 by neither width
    for io in (SRC, SRC | OUT):
        assert ok(C.byref(desc(L, C_=36, N=72, k=3)), io) == 1
        assert ok(C.byref(desc(L, C_=40, N=72, k=3)), io) == 1
        assert ok(C.byref(desc(L, C_=32, N=72, src_ld=34, k=3)), io) == 0
        assert ok(C.byref(desc(L, C_=34, N=72, k=3)), io) == 0
    # N = 45 with out_ld = 45: the scalar epilogue takes bf16 and fp32 outputs
    for io in (SRC, SRC | OUT):
        assert ok(C.byref(desc(L, C_=256, N=45, hw=10, k=3)), io) == 1
    # agreement with the fp32-in-memory predicate at io_flags = 0
    for d in (desc(L), desc(L, C_=36, N=72, k=3), desc(L, C_=32, src_ld=34)):
        assert ok(C.byref(d), 0) == L.lib.zsg_conv_igemm_bf16_supported(C.byref(d))


def test_tuning_key_and_shipped_table(Z):
    import json
    from zsgnet_pytorch_amd import ops
    tj = json.load(open(ops.SHIPPED_TABLE))
    assert tj["entries"] and not any("bf16" in k for k in tj["entries"]), "no bf16 / bf16_act entries ship: the first forward tunes"
    assert tj["source_stamp"] == ops.files_stamp()
    src = open(os.path.join(ROOT, "zsgnet-pytorch_amd", "ops.py")).read()
    assert '"bf16" if bf16 else "fp32"' in src and '":io%d" % args[5]' in src, "the io flags are part of the tuning key"


def test_ddp_wrapper_forwards_eval_precision(Z):
    from zsgnet_pytorch_amd import dist
    assert callable(getattr(dist.DistributedDataParallel, "eval_precision", None))


def test_eval_speed_lists_bf16_act():
    tool = os.path.join(ROOT, "tools", "eval_speed.py")
    r = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--dtype" in r.stdout and "bf16_act" in r.stdout
    r = subprocess.run([sys.executable, tool, "--dtype", "fp16"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "invalid choice" in r.stderr

"""cfg lang_fuse = "words" on the host (no GPU): what ZSGNet.__init__ accepts and declares (keys, flat-buffer offsets, the zero / drawn
start), checkpoint compatibility, the LAMB grouping of the new tensors, the C ABI's binding, and the host definition tests/words_ref.py —
equal to the oracle's forward at W_value = 0 in float64, differentiable as stated (gradcheck of its head on a tiny pyramid), and with the
backward formulas of include/zsg.h restated as float64 loops against autograd."""
import math

import pytest
import torch

import words_ref as WR
from oracle import zsg_oracle as O
from zsgnet_pytorch_amd import _lib, mdl, optim
from zsgnet_pytorch_amd.config import get_cfg

ARCH = "resnet18"


def make(**flags):
    return mdl.get_default_net(9, get_cfg(resnet_arch=ARCH, **flags))


def offsets(net):
    return {n: (e.offset, e.size, e.shape) for n, e in net.store.entries.items()}


def test_default_and_film_declare_nothing_new():
    assert "words" in mdl.LANG_FUSES and get_cfg()["lang_fuse"] == "concat"
    for flags in (dict(), dict(lang_fuse="concat"), dict(lang_fuse="film"), dict(lang_pool="attn"), dict(lang_fuse="film", lang_pool="mean")):
        net = make(**flags)
        assert not [k for k in net.state_dict() if "words" in k], flags
    assert set(make().state_dict().keys()) == set(O.seeded_state_dict(ARCH, 0).keys())


@pytest.mark.parametrize("same_atb", [True, False])
def test_words_adds_its_weights_behind_everything(same_atb):
    base = make(use_same_atb=same_atb, lang_pool="attn")
    net = make(use_same_atb=same_atb, lang_pool="attn", lang_fuse="words")
    stacks = ["att_reg_box"] if same_atb else ["att_box", "reg_box"]
    new = [f"{p}.words.{kv}.weight" for p in stacks for kv in ("key", "value")]
    assert set(net.state_dict().keys()) == set(base.state_dict().keys()) | set(new)
    assert net._param_names == base._param_names + new, "declared behind every existing entry, lang_pool.weight included; key then value"
    ob, on = offsets(base), offsets(net)
    assert all(on[k] == ob[k] for k in ob), "no existing offset moves"
    end = base.store.total
    for k in new:
        assert net.state_dict()[k].shape == (256, net.lstm_out_dim)
        assert on[k][0] == end
        end += 256 * net.lstm_out_dim
    assert net.store.total == end
    assert make(lang_fuse="words", lang_pool="mean", lstm_dim=32).state_dict()["att_reg_box.words.key.weight"].shape == (256, 64)
    # one direction: "final" keeps the sequence program under words (the default net falls back to "last")
    uni = make(lang_fuse="words", lang_pool="final", use_bidirectional=False)
    assert uni.lang_pool_mode == "final" and uni.state_dict()["att_reg_box.words.value.weight"].shape == (256, 128)
    assert make(lang_pool="final", use_bidirectional=False).lang_pool_mode == "last"


def test_reset_parameters_zeroes_value_draws_key_and_leaves_concat_alone():
    net = make(lang_fuse="words", lang_pool="final", use_same_atb=False)
    net.reset_parameters(seed=3)
    sd = net.state_dict()
    D = net.lstm_out_dim
    for p in ("att_box", "reg_box"):
        assert not sd[p + ".words.value.weight"].any(), "zero: a fresh words net computes concat"
        k = sd[p + ".words.key.weight"]
        assert k.any() and float(k.abs().max()) <= 1.0 / math.sqrt(D) and float(k.abs().max()) > 0.9 / math.sqrt(D)
    assert not torch.equal(sd["att_box.words.key.weight"], sd["reg_box.words.key.weight"])
    ref = make(lang_pool="final", use_same_atb=False)
    ref.reset_parameters(seed=3)
    rs = ref.state_dict()
    assert all(torch.equal(sd[k], rs[k]) for k in rs), "the new names come last: no existing parameter's draw changes"


def test_errors():
    with pytest.raises(ValueError, match="lang_fuse"):
        make(lang_fuse="Words")
    with pytest.raises(ValueError, match="lang_fuse"):
        make(lang_fuse="words")                                    # lang_pool defaults to "last"
    with pytest.raises(ValueError, match="lang_fuse"):
        make(lang_fuse="words", lang_pool="last")
    for pool in ("final", "mean", "attn"):
        with pytest.raises(ValueError, match="lang_fuse"):
            make(lang_fuse="words", lang_pool=pool, use_lang=False)
        with pytest.raises(ValueError, match="lang_fuse"):
            make(lang_fuse="words", lang_pool=pool, use_img=False)
        make(lang_fuse="words", lang_pool=pool)
    make(lang_fuse="concat", use_lang=False)


def test_concat_checkpoint_loads_into_words():
    src = make(lang_pool="mean")
    src.reset_parameters(seed=5)
    ck = {k: v.detach().clone() for k, v in src.state_dict().items()}
    net = make(lang_pool="mean", lang_fuse="words")
    net.reset_parameters(seed=6)
    with pytest.raises(RuntimeError, match="words"):
        net.load_state_dict(ck)
    res = net.load_state_dict(ck, strict=False)
    assert list(res.missing_keys) == ["att_reg_box.words.key.weight", "att_reg_box.words.value.weight"] and not res.unexpected_keys
    sd = net.state_dict()
    assert not sd["att_reg_box.words.value.weight"].any(), "stays at its zero start: the net computes what the checkpoint's did"
    assert all(torch.equal(sd[k], ck[k]) for k in ck)
    with pytest.raises(RuntimeError, match="words"):
        make(lang_pool="mean").load_state_dict({k: v.clone() for k, v in sd.items()})


def test_lamb_puts_both_weights_in_the_adaptive_group():
    net = make(lang_fuse="words", lang_pool="final", use_same_atb=False)
    named = dict(net.named_parameters())
    groups = optim.lamb_param_groups(net._ordered_params())
    assert len(groups) == 2 and groups[1].get("adapt") is False
    adaptive = {id(p) for p in groups[0]["params"]}
    for k in ("att_box.words.key.weight", "att_box.words.value.weight", "reg_box.words.key.weight", "reg_box.words.value.weight"):
        assert named[k].dim() == 2 and id(named[k]) in adaptive
        assert id(named[k]) not in {id(p) for p in groups[1]["params"]}
    assert net._ordered_params()[-1] is named["reg_box.words.value.weight"]


def test_c_abi_is_bound():
    want = {"zsg_head_words_conv0": 20, "zsg_head_words_conv0_bwd": 21, "zsg_head_words_bwd_ws_bytes": 5}
    for name, n in want.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n
    hw = torch.tensor([3, 4, 2, 2], dtype=torch.int32)
    ws = _lib.lib.zsg_head_words_bwd_ws_bytes
    assert ws(6, 5, 2, hw.data_ptr(), 8) > 0
    assert ws(6, 5, 2, hw.data_ptr(), 6) == -1 and ws(6, 5, 2, hw.data_ptr(), 1028) == -1
    assert ws(6, 0, 2, hw.data_ptr(), 8) == -1 and ws(6, 65, 2, hw.data_ptr(), 8) == -1 and ws(6, 64, 2, hw.data_ptr(), 8) > 0


def batch64(B=2, S=64, seed=4):
    bt = O.synthetic_batch(B, S, S, seed=seed)
    g = torch.Generator().manual_seed(seed)
    h0, c0 = torch.randn(2, B, 128, generator=g), torch.randn(2, B, 128, generator=g)
    return {k: v.double() for k, v in bt.items()}, h0.double(), c0.double(), O.sort_rank(bt["qlens"])


@pytest.mark.parametrize("same_atb", [True, False])
def test_reference_at_zero_value_weight_is_the_oracle(same_atb):
    """words_ref with W_value = 0 (and a drawn W_key) against oracle.zsgnet_forward in float64 (lang_pool = last, the oracle's encoder; final /
    mean against the oracle's pieces around langpool_ref's encoder): 1e-12 relative (conv0's sum is split, so not bit-equal)"""
    import langpool_ref as LR
    sd = O.seeded_state_dict(ARCH, 2)
    if not same_atb:       # separate heads from the shared one's tensors (the oracle seeds the paper's configuration)
        for k in [k for k in sd if k.startswith("att_reg_box.")]:
            v = sd.pop(k)
            tail = k[len("att_reg_box."):]
            if tail.startswith("5."):
                v5 = v.view(9, 5, *v.shape[1:])
                sd["att_box." + tail] = v5[:, 4:5].reshape(9, *v.shape[1:]).clone()
                sd["reg_box." + tail] = v5[:, :4].reshape(36, *v.shape[1:]).clone()
            else:
                sd["att_box." + tail], sd["reg_box." + tail] = v.clone(), v.flip(0).clone()
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    bt, h0, c0, rank = batch64()
    g = torch.Generator().manual_seed(9)
    stacks = ["att_reg_box."] if same_atb else ["att_box.", "reg_box."]
    for pool_mode, do_norm in (("last", False), ("last", True), ("final", False), ("mean", False)):
        with torch.no_grad():
            if pool_mode == "last":        # the oracle's own query encoder
                want = O.zsgnet_forward(sd, bt, h0, c0, arch=ARCH, rank=rank, do_norm=do_norm)
            else:                          # the oracle's pieces around tests/langpool_ref.py's query encoder
                want = LR.zsgnet_forward(sd, bt, h0, c0, arch=ARCH, rank=rank, lang_pool=pool_mode)
            sdw = dict(sd)
            for p in stacks:
                sdw[p + "words.key.weight"] = torch.randn(256, 256, generator=g, dtype=torch.float64) * 0.1
                sdw[p + "words.value.weight"] = torch.zeros(256, 256, dtype=torch.float64)
            got = WR.zsgnet_forward(sdw, bt, h0, c0, arch=ARCH, rank=rank, do_norm=do_norm, lang_pool=pool_mode)
        for k in ("att_out", "bbx_out"):
            scale = float(want[k].abs().max())
            assert float((got[k] - want[k]).abs().max()) <= 1e-12 * scale, (k, pool_mode, do_norm)
        assert got["feat_sizes"].tolist() == want["feat_sizes"].tolist()
        sdw = {k: (torch.full_like(v, 0.01) if k.endswith("words.value.weight") else v) for k, v in sdw.items()}
        with torch.no_grad():
            moved = WR.zsgnet_forward(sdw, bt, h0, c0, arch=ARCH, rank=rank, do_norm=do_norm, lang_pool=pool_mode)
        assert float((moved["bbx_out"] - want["bbx_out"]).abs().max()) > 1e-6 * float(want["bbx_out"].abs().max())


def tiny_head(C=8, D=4, T=5, seed=0):
    """a head of C channels on features of C channels, language width D, T tokens, one anchor, 5 outputs; lens 3, 0 ... T"""
    g = torch.Generator().manual_seed(seed)

    def r(*s):
        return (torch.randn(*s, generator=g, dtype=torch.float64) * 0.4).requires_grad_(True)
    sd = {"att_reg_box.0.0.weight": r(C, C + D + 2, 3, 3), "att_reg_box.0.0.bias": r(C), "att_reg_box.words.key.weight": r(C, D),
          "att_reg_box.words.value.weight": r(C, D), "att_reg_box.5.weight": r(5, C, 3, 3), "att_reg_box.5.bias": r(5)}
    for i in range(1, 5):
        sd[f"att_reg_box.{i}.0.weight"], sd[f"att_reg_box.{i}.0.bias"] = r(C, C, 3, 3), r(C)
    feats = [r(3, C, 3, 4), r(3, C, 2, 2)]
    we = r(3, D)
    o = r(3, T, D)
    return sd, feats, we, o, [3, 0, T]


def test_reference_head_gradcheck():
    """torch.autograd.gradcheck of words_ref's head stage in float64: levels 3 x 4 and 2 x 2, 8 channels, lens 3 / 0 / T"""
    sd, feats, we, o, lens = tiny_head()
    names = sorted(sd)

    def fn(f0, f1, w, oo, *params):
        s = dict(zip(names, params))
        return torch.cat([WR.words_head(s, f, w, oo, lens) for f in (f0, f1)], dim=1)
    assert torch.autograd.gradcheck(fn, (feats[0], feats[1], we, o) + tuple(sd[n] for n in names), eps=1e-6, atol=1e-6, rtol=1e-4)


def test_padding_tokens_do_not_matter():
    sd, feats, we, o, lens = tiny_head(seed=3)
    with torch.no_grad():
        a = WR.words_head(sd, feats[0], we, o, lens)
        o2 = o.clone()
        o2[0, 3:] = 7.0
        o2[1] = -3.0
        assert torch.equal(a, WR.words_head(sd, feats[0], we, o2, lens))


def test_backward_formulas_agree_with_autograd():
    """the float64 loops restating include/zsg.h's backward of zsg_head_words_conv0 against autograd of words_ref's h1"""
    sd, feats, we, o, lens = tiny_head(seed=5)
    f = feats[0]
    B, C, h, w = f.shape
    T = o.shape[1]
    c = 1.0 / math.sqrt(C)
    Wk, Wv = sd["att_reg_box.words.key.weight"], sd["att_reg_box.words.value.weight"]
    Kw = (o @ Wk.t()).detach().requires_grad_(True)
    Vw = (o @ Wv.t()).detach().requires_grad_(True)
    import torch.nn.functional as F
    W0, b0 = sd["att_reg_box.0.0.weight"].detach(), sd["att_reg_box.0.0.bias"].detach()
    Y = F.conv2d(f.detach(), W0[:, :C], None, 1, 1).requires_grad_(True)
    rest = F.conv2d(O.fuse_lang_grid(f.detach(), we.detach())[:, C:], W0[:, C:], None, 1, 1) + b0[None, :, None, None]
    gamma, alpha = WR.attention(Y, Kw, Vw, lens, c)
    h1 = F.relu((1 + gamma) * Y + rest)
    gup = torch.randn(h1.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    h1.backward(gup)
    dy = (gup * (h1 > 0)).detach().permute(0, 2, 3, 1).reshape(B, h * w, C)        # the ReLU-masked gradient, rows [p][n]
    Yr = Y.detach().permute(0, 2, 3, 1).reshape(B, h * w, C)
    dYq, dKw, dVw = torch.zeros_like(Yr), torch.zeros(B, T, C, dtype=torch.float64), torch.zeros(B, T, C, dtype=torch.float64)
    for b in range(B):
        n = lens[b]
        for p in range(h * w):
            a = alpha[b, p].detach()
            assert not a[n:].any() and (n == 0 or abs(float(a.sum()) - 1) < 1e-12)
            dgam = dy[b, p] * Yr[b, p]
            dal = torch.stack([dgam @ Vw[b, t].detach() for t in range(n)]) if n else torch.zeros(0, dtype=torch.float64)
            dot = sum(float(a[k]) * float(dal[k]) for k in range(n))
            ds = [float(a[t]) * (float(dal[t]) - dot) for t in range(n)]
            gam = sum((a[t] * Vw[b, t].detach() for t in range(n)), torch.zeros(C, dtype=torch.float64))
            dYq[b, p] = (1 + gam) * dy[b, p] + c * sum((ds[t] * Kw[b, t].detach() for t in range(n)), torch.zeros(C, dtype=torch.float64))
            for t in range(n):
                dKw[b, t] += c * ds[t] * Yr[b, p]
                dVw[b, t] += float(a[t]) * dgam
    gY = Y.grad.permute(0, 2, 3, 1).reshape(B, h * w, C)
    assert float((dYq - gY).abs().max()) <= 1e-12 * max(1.0, float(gY.abs().max()))
    assert float((dKw - Kw.grad).abs().max()) <= 1e-12 * max(1.0, float(Kw.grad.abs().max()))
    assert float((dVw - Vw.grad).abs().max()) <= 1e-12 * max(1.0, float(Vw.grad.abs().max()))
    assert not Kw.grad[0, 3:].any() and not Kw.grad[1].any() and not Vw.grad[1].any() and Kw.grad[2].any() and Vw.grad[0, :3].any()

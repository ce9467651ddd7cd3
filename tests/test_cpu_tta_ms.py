"""Multi-scale test-time augmentation and box voting (cfg eval_scales / eval_box_vote) without a GPU: the cfg keys and their validation,
ZSGNet.eval_scales and the data-parallel wrapper, the size rule, the concatenated anchor table, the new symbols in include/zsg.h and the
ctypes table, and the properties of the definition tests/vote_ref.py that the GPU parity test relies on."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topk_ref  # noqa: E402
import tta_ms_ref as MS  # noqa: E402
import vote_ref  # noqa: E402
from oracle import zsg_oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def Z():
    from zsgnet_pytorch_amd import _lib, config, evaluator, mdl
    return _lib, config, mdl, evaluator


# ---- the switches ----------------------------------------------------------------------------------------------------------------------------
def test_cfg_keys_defaults_and_where_they_are_applied(Z):
    _, config, mdl, evaluator = Z
    cfg = config.get_cfg()
    assert cfg["eval_scales"] == [] and cfg["eval_box_vote"] == 0.0
    assert config.update_from_dict(config.get_cfg(), {"eval_scales": "[0.75, 1.25]", "eval_box_vote": "0.6"})["eval_scales"] == [0.75, 1.25]
    net = mdl.get_default_net(9, config.get_cfg(eval_scales=[0.75, 1.25], resnet_arch="resnet18"))
    assert net._eval_scales == (0.75, 1.25)
    assert mdl.get_default_net(9, config.get_cfg(resnet_arch="resnet18"))._eval_scales == ()
    cfg = config.get_cfg(resnet_arch="resnet18")
    del cfg["eval_scales"], cfg["eval_box_vote"]
    assert mdl.get_default_net(9, cfg)._eval_scales == (), "a cfg without the key = the default"
    r, s = config.ratios_scales(cfg)
    ev = evaluator.get_default_eval(r, s, cfg)
    assert ev.box_vote == 0.0 and ev.met_keys == ["Acc", "MaxPos"]
    assert evaluator.get_default_eval(r, s, config.get_cfg(eval_box_vote=0.6)).box_vote == 0.6
    assert evaluator.get_default_eval(r, s, config.get_cfg(eval_box_vote=1)).box_vote == 1.0
    with pytest.raises(ValueError, match="eval_scales"):
        mdl.get_default_net(9, config.get_cfg(eval_scales=[0.25], resnet_arch="resnet18"))


@pytest.mark.parametrize("bad", [[0.6, 0.7, 0.8, 0.9, 1.1], [0.49], [2.01], [float("nan")], [float("inf")], ["0.75"], [None], [True], 0.75, "0.75",
                                 [[0.75]]])
def test_bad_eval_scales_raise(Z, bad):
    _, config, mdl, _ = Z
    net = mdl.get_default_net(9, config.get_cfg(resnet_arch="resnet18")).eval_scales([1.5])
    with pytest.raises(ValueError, match="eval_scales"):
        net.eval_scales(bad)
    assert net._eval_scales == (1.5,), "a refused value changes nothing"


@pytest.mark.parametrize("bad", [-0.1, 1.01, float("nan"), float("inf"), "0.5", None, True, [0.5]])
def test_bad_eval_box_vote_raises(Z, bad):
    _, config, _, evaluator = Z
    cfg = config.get_cfg()
    cfg["eval_box_vote"] = bad
    with pytest.raises(ValueError, match="eval_box_vote"):
        evaluator.get_default_eval(*config.ratios_scales(cfg), cfg)


def test_setter_returns_self_and_the_wrapper_passes_it_through(Z):
    _, config, mdl, _ = Z
    from zsgnet_pytorch_amd import dist as zdist
    net = mdl.get_default_net(9, config.get_cfg(resnet_arch="resnet18"))
    assert net.eval_scales([0.5, 2]) is net and net._eval_scales == (0.5, 2.0)
    assert net.eval_scales() is net and net._eval_scales == ()
    ddp = object.__new__(zdist.DistributedDataParallel)
    torch.nn.Module.__init__(ddp)
    ddp.module = net
    assert ddp.eval_scales((0.75,)) is ddp and net._eval_scales == (0.75,)
    with pytest.raises(ValueError, match="eval_scales"):
        ddp.eval_scales([3.0])


def test_size_rule(Z):
    _, _, mdl, _ = Z
    assert mdl.eval_scale_sizes(128, 128, [0.75, 1.25]) == [(96, 96), (160, 160)] == MS.scale_sizes(128, 128, [0.75, 1.25])
    assert mdl.eval_scale_sizes(300, 300, [0.75, 1.25]) == [(225, 225), (375, 375)]
    assert mdl.eval_scale_sizes(10, 30, [0.75, 0.85]) == [(8, 23), (9, 26)], "halves round up: 7.5 -> 8, 22.5 -> 23, 8.5 -> 9, 25.5 -> 26"
    for H, W, sc in ((128, 96, [0.5, 2.0, 1.1]), (301, 299, [0.9, 1.7])):
        assert mdl.eval_scale_sizes(H, W, sc) == MS.scale_sizes(H, W, sc)
    with pytest.raises(ValueError, match="eval_scales.*own size"):
        mdl.eval_scale_sizes(128, 128, [0.75, 1.0])
    with pytest.raises(ValueError, match="eval_scales.*own size"):
        mdl.eval_scale_sizes(128, 128, [1.003])
    with pytest.raises(ValueError, match="eval_scales.*both round"):
        mdl.eval_scale_sizes(128, 128, [0.75, 0.751])


def test_import_direction_and_new_symbols(Z):
    L, _, _, _ = Z
    src = open(os.path.join(ROOT, "zsgnet-pytorch_amd", "mdl.py")).read()
    assert not re.search(r"^(from|import) .*dat_loader", src, re.M), "mdl.py imports the resizer where it is used, not at import time"
    P, I32, F32_, SZ = L.P, L.I32, L.F32, L.SZ
    assert L.SIGNATURES["zsg_eval_vote_workspace_bytes"] == (SZ, [I32, I32, I32, I32])
    assert L.SIGNATURES["zsg_eval_vote"] == (I32, [P, P, P, P, I32, I32, I32, I32, F32_, F32_, P, P, P, P, P, P, P, P, P, SZ, P])
    hdr = open(os.path.join(ROOT, "include", "zsg.h")).read()
    assert "int zsg_eval_vote(" in hdr and "size_t zsg_eval_vote_workspace_bytes(" in hdr
    assert "vote.hip" in open(os.path.join(ROOT, "zsgnet-pytorch_amd", "csrc", "Makefile")).read()
    assert L.lib.zsg_eval_vote_workspace_bytes(16, 17460, 128, 5) == L.lib.zsg_eval_topk_workspace_bytes(16, 17460, 128, 5)
    p = 4096                                                       # refused before anything could be launched: no GPU is needed
    ok = [p, None, p, p, 2, 100, 128, 5, 0.5, 0.5, p, p, p, p, p, p, None, None, p, 1 << 20, None]
    for i, v in ((0, None), (2, None), (13, None), (14, None), (15, None), (18, None), (4, 0), (6, 600), (7, 65), (8, 0.0), (8, 1.5), (19, 8)):
        bad = list(ok)
        bad[i] = v
        assert L.lib.zsg_eval_vote(*bad) == -1, (i, v)
    bad = list(ok)
    bad[16] = p                                                    # hit_rank without annot
    assert L.lib.zsg_eval_vote(*bad) == -1 and b"annot" in L.lib.zsg_last_error()


# ---- the concatenated anchor table -----------------------------------------------------------------------------------------------------------
def test_pooled_anchor_table(Z):
    _, config, _, evaluator = Z
    cfg = config.get_cfg()
    r, s = config.ratios_scales(cfg)
    fs = [O.feat_sizes_for(128, 128), O.feat_sizes_for(96, 96), O.feat_sizes_for(160, 160)]
    tab = MS.pooled_anchors(fs, r, s)
    A = [sum(h * w * 9 for h, w in f) for f in fs]
    assert tab.shape == (sum(A), 4) and len(set(A)) == 3
    from zsgnet_pytorch_amd.anchors import create_anchors
    own = create_anchors(fs[0], ratios=r, scales=s, flatten=True, device="cpu").numpy()
    assert np.array_equal(tab[:A[0]], own.astype(F32)), "pass 0's rows are create_anchors' own"
    assert np.array_equal(tab[A[0]:A[0] + A[1]], create_anchors(fs[1], ratios=r, scales=s, flatten=True, device="cpu").numpy().astype(F32))
    # the evaluator builds the same table from the dict's tta_feat_sizes and leaves self.anchs the pass-0 table
    ev = evaluator.get_default_eval(r, s, cfg)
    out = dict(att_bbx_out=torch.zeros(1, A[0], 5), feat_sizes=torch.tensor(fs[0]), tta_att_bbx_out=torch.zeros(1, sum(A), 5), tta_feat_sizes=fs)
    o5, anchs = ev._out5_anchors(out)
    assert tuple(o5.shape) == (1, sum(A), 5) and np.array_equal(anchs.numpy(), tab) and np.array_equal(ev.anchs.numpy(), own)
    assert ev._out5_anchors(out)[1] is anchs, "cached per size tuple"
    o5, anchs = ev._out5_anchors({k: v for k, v in out.items() if not k.startswith("tta_")})
    assert tuple(o5.shape) == (1, A[0], 5) and anchs is ev.anchs


# ---- the definition of the vote --------------------------------------------------------------------------------------------------------------
def _boxes_case(boxes_norm, logits, img=(200.0, 400.0)):
    """candidates given as decoded boxes: anchors = the boxes, regressions zero"""
    anc = np.asarray(boxes_norm, F32)
    att = np.asarray(logits, F32)[None]
    return att, np.zeros((1, anc.shape[0], 4), F32), np.array([img], F32), anc


def test_hand_computed_three_boxes():
    # two boxes that overlap with IoU 0.6 / (0.8 + 0.8 - 0.6) = 0.6 and one far away; logits ln 3, 0, ln 3 -> scores 0.75, 0.5, 0.75
    att, reg, sz, anc = _boxes_case([[-0.5, -0.5, 0.5, 0.3], [-0.5, -0.3, 0.5, 0.5], [0.6, 0.6, 0.9, 0.9]], [np.log(3.0), 0.0, np.log(3.0)])
    r = vote_ref.vote(att, reg, None, sz, anc, pre_n=3, K=3, vote_thr=0.55, nms_thr=0.7)
    assert r["topk_idx"].tolist() == [[0, 2, 1]] and r["vote_n"].tolist() == [[2, 1, 2]]
    px = topk_ref.to_pixels(anc, np.broadcast_to(sz[0], (3, 2)))          # x1y1x2y2: [100, 50, 260, 150], [140, 50, 300, 150], [320, 160, 380, 190]
    np.testing.assert_allclose(px, [[100, 50, 260, 150], [140, 50, 300, 150], [320, 160, 380, 190]], rtol=1e-6)
    s = O._sigmoid(att)[0].astype(np.float64)
    want0 = (s[0] * px[0] + s[1] * px[1]) / (s[0] + s[1])                 # (0.75 * 100 + 0.5 * 140) / 1.25 = 116 ...
    np.testing.assert_allclose(want0, [116, 50, 276, 150], rtol=1e-6)
    np.testing.assert_allclose(r["vote_boxes"][0, 0], want0, rtol=1e-6)
    assert np.array_equal(r["vote_boxes"][0, 1], r["topk_boxes"][0, 1])   # alone: its own box, bit for bit
    np.testing.assert_allclose(r["vote_boxes"][0, 2], want0, rtol=1e-6)   # row 2 (anchor 1) has the same two members: the same box
    assert np.array_equal(r["topk_scores"], O._sigmoid(att)[:, [0, 2, 1]])
    # a threshold above their IoU: nobody votes with anybody
    r = vote_ref.vote(att, reg, None, sz, anc, pre_n=3, K=3, vote_thr=0.65, nms_thr=0.7)
    assert r["vote_n"].tolist() == [[1, 1, 1]] and np.array_equal(r["vote_boxes"], r["topk_boxes"])


def _random_case(seed=0, A=200, B=2):
    ratios, scales = O.default_ratios_scales()
    anc = O.create_anchors([(4, 4), (2, 2)], ratios, scales).astype(F32)[:A]
    g = np.random.default_rng(seed)
    att = (g.standard_normal((B, anc.shape[0])) * 1.5 - 2).astype(F32)
    reg = (g.standard_normal((B, anc.shape[0], 4)) * 0.1).astype(F32)
    annot = np.array([[-0.5, -0.5, 0.5, 0.5]] * B, F32)
    return att, reg, annot, np.array([[300, 400]] * B, F32), anc


def test_threshold_one_with_distinct_boxes_is_the_identity():
    att, reg, annot, sz, anc = _random_case()
    r = vote_ref.vote(att, reg, annot, sz, anc, pre_n=64, K=5, vote_thr=1.0)
    assert (r["vote_n"] == 1).all() and np.array_equal(r["vote_boxes"], r["topk_boxes"])
    assert np.array_equal(r["vote_hit_rank"], r["hit_rank"]) and np.array_equal(r["vote_acc_at"], r["acc_at"])


def test_candidates_outside_pre_n_do_not_matter():
    att, reg, annot, sz, anc = _random_case(1)
    a = vote_ref.vote(att, reg, annot, sz, anc, pre_n=16, K=3, vote_thr=0.5)
    assert a["vote_n"].max() > 1
    rest = np.argsort(-att, axis=1, kind="stable")[:, 16:]
    att2, reg2 = att.copy(), reg.copy()
    for b in range(att.shape[0]):
        att2[b, rest[b]] -= 5.0                                    # still below every candidate, now with other scores and boxes
        reg2[b, rest[b]] = 0.3
    b_ = vote_ref.vote(att2, reg2, annot, sz, anc, pre_n=16, K=3, vote_thr=0.5)
    for k in ("vote_boxes", "vote_n", "topk_idx", "vote_hit_rank"):
        assert np.array_equal(a[k], b_[k]), k


def test_a_nan_score_never_contributes():
    att, reg, annot, sz, anc = _random_case(2)
    a = vote_ref.vote(att, reg, annot, sz, anc, pre_n=200, K=3, vote_thr=0.5)
    assert a["vote_n"].max() > 1
    members = a["vote_n"].copy()
    # with pre_n = A every anchor is a candidate: NaN scores rank last, are candidates all the same, and change nothing
    low = np.argsort(att, axis=1)[:, :20]
    att2, reg2 = att.copy(), reg
    for b in range(att.shape[0]):
        att2[b, [i for i in low[b] if i not in a["topk_idx"][b]]] = np.nan
    n = vote_ref.vote(att2, reg2, annot, sz, anc, pre_n=200, K=3, vote_thr=0.5)
    assert np.array_equal(n["topk_idx"], a["topk_idx"]) and (n["vote_n"] <= members).all()
    # the voted boxes are the sums without those candidates: the same call on the arrays without them
    for b in range(att.shape[0]):
        keep = np.array([i for i in range(att.shape[1]) if not np.isnan(att2[b, i])])
        sub = vote_ref.vote(att2[b:b + 1, keep], reg2[b:b + 1, keep], annot[b:b + 1], sz[b:b + 1], anc[keep], pre_n=len(keep), K=3, vote_thr=0.5)
        assert np.array_equal(sub["vote_boxes"][0], n["vote_boxes"][b]) and np.array_equal(sub["vote_n"][0], n["vote_n"][b])
    # a row that is NaN itself (every score NaN): kept as the NMS left it, no member
    allnan = vote_ref.vote(np.full_like(att, np.nan), reg, annot, sz, anc, pre_n=8, K=2, vote_thr=0.5)
    assert (allnan["vote_n"] == 0).all() and np.array_equal(allnan["vote_boxes"], allnan["topk_boxes"])

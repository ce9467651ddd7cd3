"""What "correct" means for shared-image training, pinned on the CPU in float64 before any GPU code is trusted: the shared forward
composed from the oracle's pieces (tests/shared_train_ref.py: the trunk once per distinct image, the feature maps indexed by img_idx)
must agree with oracle.zsgnet_forward on the expanded batch img[img_idx] — outputs, loss and every gradient, relative 1e-9 —
  * for EQUAL groups in train mode (every image has the same number of queries: train-mode BatchNorm then sees the same statistics),
  * for ANY groups with training=False (frozen BatchNorm),
  * for ssd_vgg (no BatchNorm) with any groups.
The bound: float64 rounding through tiny-batch BatchNorm leaves about 1e-13; 1e-9 keeps room and still separates the case that is a
DIFFERENT function — unequal groups with train-mode BatchNorm, where the expanded batch weights an image's pixels by its query count
(checked last: the two differ by far more than any rounding)."""
import numpy as np
import pytest
import torch

from oracle import zsg_oracle as O
from shared_train_ref import as_fp64, shared_forward, want_grads
from zsgnet_pytorch_amd import synth

RATIOS, SCALES = O.default_ratios_scales()


def rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-300))


def both(arch, hw, idx, training, seed=3):
    Bi, Q = max(idx) + 1, len(idx)
    bt = synth.synthetic_shared_batch(Bi, Q, hw, hw, seed=17, tmax=9)
    bt["img_idx"] = torch.tensor(idx, dtype=torch.long)
    g = torch.Generator().manual_seed(5)
    h0, c0 = torch.randn(2, Q, 128, generator=g).double(), torch.randn(2, Q, 128, generator=g).double()
    sd = O.seeded_ssd_state_dict(seed) if arch == "ssd_vgg" else O.seeded_state_dict(arch, seed)
    want_grads(sd)
    rank = O.sort_rank(bt["qlens"])
    res = []
    for shared in (True, False):
        sd64, bt64 = as_fp64(sd, bt)
        if shared:
            out = shared_forward(sd64, bt64, h0, c0, arch=arch, training=training, rank=rank)
        else:
            out = O.zsgnet_forward(sd64, synth.expand_shared(bt64), h0, c0, arch=arch, training=training, rank=rank)
        fs = [tuple(r) for r in out["feat_sizes"].tolist()]
        anc = torch.from_numpy(O.create_anchors(fs, RATIOS, SCALES).astype(np.float32))
        ls = O.torch_loss(out, bt["annot"], anc)
        ls["loss"].backward()
        res.append((sd64, out, ls))
    return res


def distances(res):
    (sa, oa, la), (sb, ob, lb) = res
    d = dict(att=rel(oa["att_out"].detach(), ob["att_out"].detach()), bbx=rel(oa["bbx_out"].detach(), ob["bbx_out"].detach()),
             loss=abs(float(la["loss"]) - float(lb["loss"])) / abs(float(lb["loss"])))
    worst = 0.0
    for k, v in sb.items():
        if v.is_floating_point() and v.requires_grad and v.grad is not None:
            assert sa[k].grad is not None, k
            worst = max(worst, rel(sa[k].grad, v.grad))
    d["grad"] = worst
    return d


@pytest.mark.parametrize("arch,hw,idx,training", [
    ("resnet18", 96, [1, 0, 2, 0, 2, 1], True),
    ("resnet18", 96, [1, 0, 2, 0, 2, 1, 1, 1], False),
    ("ssd_vgg", 300, [1, 0, 0, 1, 0], True),
], ids=["r18_equal_groups_train", "r18_unequal_groups_frozen_bn", "ssd_vgg_unequal_groups"])
def test_composed_shared_oracle_agrees_with_the_expanded_batch(arch, hw, idx, training):
    res = both(arch, hw, idx, training)
    d = distances(res)
    print(f"shared vs expanded, fp64, {arch} {hw}^2 idx {idx} training={training}: {d}")
    assert max(d.values()) <= 1e-9, d
    if arch != "ssd_vgg" and training:
        # running_mean equal; running_var differs only through the unbiased factor n / (n - 1), n = B * H * W of each batch
        (sa, _, _), (sb, _, _) = res
        k = "backbone.encoder.bn1.running_mean"
        assert rel(sa[k], sb[k]) <= 1e-9
        assert int(sa["backbone.encoder.bn1.num_batches_tracked"]) == int(sb["backbone.encoder.bn1.num_batches_tracked"]) == 1


def test_unequal_groups_with_train_mode_batchnorm_are_a_different_function():
    d = distances(both("resnet18", 96, [1, 0, 2, 0, 2, 1, 1, 1], True))
    print(f"shared vs expanded, fp64, unequal groups, train-mode BatchNorm: {d}")
    assert d["att"] > 1e-3 and d["grad"] > 1e-3, "expected two different functions (the statistics weight images differently)"

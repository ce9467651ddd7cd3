"""The reference the shared-image TRAINING tests measure against (not a test module): the shared forward composed from the oracle's
public pieces — the query encoder on the Q queries, the image trunk on the Bi distinct images, the feature maps indexed by img_idx,
then the head exactly as oracle.zsgnet_forward builds it."""
import torch

from oracle import zsg_oracle as O


def shared_forward(sd, bt, h0, c0, arch="resnet50", training=True, do_norm=False, rank=None):
    """bt: img [Bi, 3, H, W], img_idx [Q], the per-query fields with leading dimension Q.  Train-mode BatchNorm sees the Bi images, each
    once.  Returns what O.zsgnet_forward returns, with leading dimension Q."""
    bn = O.BNState(sd, training)
    we = O.query_encoder(sd, bt["qvec"], bt["qlens"], h0, c0, rank)
    if arch == "ssd_vgg":
        feats = O.ssd_forward(sd, bt["img"], False)
    else:
        c3, c4, c5 = O.encoder_forward(sd, bt["img"], arch, bn)
        feats = O.fpn_forward(sd, c3, c4, c5, False)
    wn = we
    if do_norm:
        feats = [f / f.norm(dim=1, keepdim=True) for f in feats]
        wn = we / we.norm(dim=1, keepdim=True)
    idx = bt["img_idx"].long()
    xs = [O.head_input(f.index_select(0, idx), wn, True, True) for f in feats]
    if "att_reg_box.5.weight" in sd:
        ab = torch.cat([O.head_forward(sd, x) for x in xs], dim=1)
        att, bbx = ab[..., 4:5], ab[..., :4]
    else:
        att = torch.cat([O.head_forward(sd, x, "att_box.", 1) for x in xs], dim=1)
        bbx = torch.cat([O.head_forward(sd, x, "reg_box.", 4) for x in xs], dim=1)
    return dict(att_out=att, bbx_out=bbx, feat_sizes=torch.tensor([[f.shape[2], f.shape[3]] for f in feats]),
                num_f_out=torch.tensor([len(feats)]), we=we, feats=feats)


def as_fp64(sd, bt):
    """(state dict, batch) in float64; the floating-point entries that required a gradient are fresh leaves"""
    sd64 = {k: (v.detach().double().requires_grad_(v.requires_grad) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    bt64 = {k: (v if k == "img_idx" else v.double()) for k, v in bt.items()}
    return sd64, bt64


def want_grads(sd):
    for k, v in sd.items():
        if v.is_floating_point() and "running" not in k:
            v.requires_grad_()
    return sd

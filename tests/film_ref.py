"""Host definition of cfg lang_fuse = "film": plain torch, any dtype, differentiable.

The head's first convolution of the reference sees [features | language vector | grid] and is linear in each part, so
    conv(x, W0) = conv(F, W0[:, :Cf]) + conv([lang | grid], W0[:, Cf:]).
FiLM scales the feature part per query and channel before the bias and the ReLU:
    gamma[b][n] = sum_c Wg[n][c] * we[b][c]                            Wg = sd["<head>film.weight"] [256, D]
    h1 = relu((1 + gamma)[:, :, None, None] * conv(F, W0[:, :Cf]) + conv([lang | grid], W0[:, Cf:]) + bias)
followed by the five remaining convolutions of oracle.zsg_oracle.head_forward.  With Wg = 0 this is the oracle's head up to the split of
conv0's sum.  With do_norm, `we` is the normalised vector the concatenation reads (the scale sees what the shift sees).
zsgnet_forward composes the oracle's pieces (encoder_forward, fpn_forward) and tests/langpool_ref.py's query encoder, as that file does."""
import torch
import torch.nn.functional as F

import langpool_ref as LR
from oracle import zsg_oracle as O


def film_head(sd, feat, we, prefix="att_reg_box.", outc=5):
    """One 6-convolution head on one pyramid level: feat [B, Cf, h, w], we [B, D] -> [B, h*w*A, outc]"""
    B, Cf, h, w = feat.shape
    W0, b0 = sd[prefix + "0.0.weight"], sd[prefix + "0.0.bias"]
    rest = O.fuse_lang_grid(feat, we)[:, Cf:]                     # [lang | grid] exactly as the concatenation builds them
    y = F.conv2d(feat, W0[:, :Cf], None, 1, 1)
    gamma = we @ sd[prefix + "film.weight"].t()                    # [B, 256]
    x = F.relu((1 + gamma)[:, :, None, None] * y + F.conv2d(rest, W0[:, Cf:], None, 1, 1) + b0[None, :, None, None])
    for i in range(1, 5):
        x = F.relu(F.conv2d(x, sd[f"{prefix}{i}.0.weight"], sd[f"{prefix}{i}.0.bias"], 1, 1))
    x = F.conv2d(x, sd[prefix + "5.weight"], sd[prefix + "5.bias"], 1, 1)
    return x.permute(0, 2, 3, 1).contiguous().view(B, -1, outc)


def heads(sd, feats, we):
    """(att [B, A, 1], bbx [B, A, 4]) over all levels"""
    if "att_reg_box.5.weight" in sd:
        ab = torch.cat([film_head(sd, f, we) for f in feats], dim=1)
        return ab[..., 4:5], ab[..., :4]
    att = torch.cat([film_head(sd, f, we, "att_box.", 1) for f in feats], dim=1)
    bbx = torch.cat([film_head(sd, f, we, "reg_box.", 4) for f in feats], dim=1)
    return att, bbx


def zsgnet_forward(sd, batch, h0, c0, arch="resnet50", training=True, six_hundred=False, rank=None, do_norm=False, bidirectional=True,
                   lang_pool="last"):
    """oracle.zsg_oracle.zsgnet_forward for the ResNet-FPN trunk with the FiLM head (use_lang and use_img: film needs both)"""
    bn = O.BNState(sd, training)
    we = LR.query_encoder(sd, batch["qvec"], batch["qlens"], h0, c0, rank, bidirectional, lang_pool)
    c3, c4, c5 = O.encoder_forward(sd, batch["img"], arch, bn)
    feats = O.fpn_forward(sd, c3, c4, c5, six_hundred)
    wn = we
    if do_norm:
        feats = [f / f.norm(dim=1, keepdim=True) for f in feats]
        wn = we / we.norm(dim=1, keepdim=True)
    att, bbx = heads(sd, feats, wn)
    return dict(att_out=att, bbx_out=bbx, feat_sizes=torch.tensor([[f.shape[2], f.shape[3]] for f in feats]),
                num_f_out=torch.tensor([len(feats)]), we=we, feats=feats)

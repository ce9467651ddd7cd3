"""Host definition of cfg head_ctx = "gc": plain torch, any dtype, forward only (the backward is autograd's).

A global-context block (GCNet, Cao et al. 2019) behind the heads' first convolution.  Per sample b and pyramid level, over the rows
x_p (p < P = h * w, N = 256 channels) of the post-ReLU h1, with M = N / 4:
    s_p = k . x_p                          alpha = softmax_p(s)   (max subtracted)
    c   = sum_p alpha_p x_p
    u   = W1 c + b1                        uh = (u - mean u) / sqrt(var u + 1e-5)   (biased variance over M)
    r   = relu(gamma * uh + beta)          t = W2 r + b2
    y_p = x_p + t                          (y feeds <head>.1.0 in place of h1)
k = sd["<head>gc.key.weight"] [1, N], W1 / b1 = gc.fc1, gamma / beta = gc.ln, W2 / b2 = gc.fc2.  With W2 = 0 and b2 = 0 this is the
oracle's head.  zsgnet_forward composes the oracle's pieces and tests/langpool_ref.py's query encoder, as tests/film_ref.py does;
lang_fuse = "film" takes that file's h1 in front of the block."""
import torch
import torch.nn.functional as F

import langpool_ref as LR
from oracle import zsg_oracle as O

NAMES = ("key.weight", "fc1.weight", "fc1.bias", "ln.weight", "ln.bias", "fc2.weight", "fc2.bias")


def gc_rows(x, key, W1, b1, lnw, lnb, W2, b2, eps=1e-5):
    """x [..., P, N] -> (y [..., P, N], c [..., N]): the block over the P rows of every leading index"""
    s = x @ key.reshape(-1)                                            # [..., P]
    alpha = torch.softmax(s - s.max(dim=-1, keepdim=True).values.detach(), dim=-1)
    c = (alpha.unsqueeze(-1) * x).sum(dim=-2)                          # [..., N]
    u = c @ W1.t() + b1
    mu = u.mean(dim=-1, keepdim=True)
    var = ((u - mu) ** 2).mean(dim=-1, keepdim=True)
    uh = (u - mu) / torch.sqrt(var + eps)
    r = F.relu(lnw * uh + lnb)
    t = r @ W2.t() + b2
    return x + t.unsqueeze(-2), c


def gc_map(sd, h1, prefix="att_reg_box."):
    """h1 [B, N, h, w] (post-ReLU) -> y [B, N, h, w]"""
    B, N, h, w = h1.shape
    rows = h1.permute(0, 2, 3, 1).reshape(B, h * w, N)
    y, _ = gc_rows(rows, *[sd[prefix + "gc." + n] for n in NAMES])
    return y.reshape(B, h, w, N).permute(0, 3, 1, 2)


def conv0(sd, feat, we, prefix, lang_fuse="concat", use_lang=True, use_img=True):
    """h1 of one level: the oracle's concatenation (or its blind variants), or film_ref's scaled feature part"""
    W0, b0 = sd[prefix + "0.0.weight"], sd[prefix + "0.0.bias"]
    if lang_fuse == "concat":
        return F.relu(F.conv2d(O.head_input(feat, we, use_lang, use_img), W0, b0, 1, 1))
    assert lang_fuse == "film" and use_lang and use_img
    Cf = feat.shape[1]
    rest = O.fuse_lang_grid(feat, we)[:, Cf:]
    gamma = we @ sd[prefix + "film.weight"].t()
    return F.relu((1 + gamma)[:, :, None, None] * F.conv2d(feat, W0[:, :Cf], None, 1, 1) + F.conv2d(rest, W0[:, Cf:], None, 1, 1) + b0[None, :, None, None])


def gc_head(sd, feat, we, prefix="att_reg_box.", outc=5, lang_fuse="concat", use_lang=True, use_img=True):
    """One 6-convolution head with the block behind conv0 on one pyramid level: feat [B, Cf, h, w], we [B, D] -> [B, h*w*A, outc]"""
    B = feat.shape[0]
    x = gc_map(sd, conv0(sd, feat, we, prefix, lang_fuse, use_lang, use_img), prefix)
    for i in range(1, 5):
        x = F.relu(F.conv2d(x, sd[f"{prefix}{i}.0.weight"], sd[f"{prefix}{i}.0.bias"], 1, 1))
    x = F.conv2d(x, sd[prefix + "5.weight"], sd[prefix + "5.bias"], 1, 1)
    return x.permute(0, 2, 3, 1).contiguous().view(B, -1, outc)


def heads(sd, feats, we, lang_fuse="concat", use_lang=True, use_img=True):
    """(att [B, A, 1], bbx [B, A, 4]) over all levels"""
    kw = dict(lang_fuse=lang_fuse, use_lang=use_lang, use_img=use_img)
    if "att_reg_box.5.weight" in sd:
        ab = torch.cat([gc_head(sd, f, we, **kw) for f in feats], dim=1)
        return ab[..., 4:5], ab[..., :4]
    att = torch.cat([gc_head(sd, f, we, "att_box.", 1, **kw) for f in feats], dim=1)
    bbx = torch.cat([gc_head(sd, f, we, "reg_box.", 4, **kw) for f in feats], dim=1)
    return att, bbx


def zsgnet_forward(sd, batch, h0, c0, arch="resnet50", training=True, six_hundred=False, rank=None, do_norm=False, bidirectional=True,
                   lang_pool="last", lang_fuse="concat", use_lang=True, use_img=True):
    """oracle.zsg_oracle.zsgnet_forward for the ResNet-FPN trunk with the global-context block in the heads"""
    bn = O.BNState(sd, training)
    we = LR.query_encoder(sd, batch["qvec"], batch["qlens"], h0, c0, rank, bidirectional, lang_pool)
    c3, c4, c5 = O.encoder_forward(sd, batch["img"], arch, bn)
    feats = O.fpn_forward(sd, c3, c4, c5, six_hundred)
    wn = we
    if do_norm:
        feats = [f / f.norm(dim=1, keepdim=True) for f in feats]
        wn = we / we.norm(dim=1, keepdim=True)
    att, bbx = heads(sd, feats, wn, lang_fuse, use_lang, use_img)
    return dict(att_out=att, bbx_out=bbx, feat_sizes=torch.tensor([[f.shape[2], f.shape[3]] for f in feats]),
                num_f_out=torch.tensor([len(feats)]), we=we, feats=feats)

"""Host definition of cfg lang_fuse = "words": plain torch, any dtype, differentiable.

film_ref's scale becomes a function of the pixel.  With o[b][t] (t < len_b) the BiLSTM's padded output (tests/langpool_ref.py's
lstm_outputs: the RAW output, also under do_norm), Wk / Wv = sd["<head>words.key.weight"] / sd["<head>words.value.weight"] [256, D],
N = 256 and c = 1 / sqrt(N), per pyramid level:
    Y  = conv(F, W0[:, :Cf])                                            conv0's raw feature accumulator [B, N, h, w]
    Kw[b][t] = Wk . o[b][t]         Vw[b][t] = Wv . o[b][t]
    s[b][p][t] = c * sum_n Y[b][n][p] * Kw[b][t][n]                     the accumulator row is the pixel's attention query
    alpha[b][p] = softmax over t < len_b of s (max subtracted);  0 at t >= len_b;  len_b = 0: alpha = 0
    gamma[b][n][p] = sum_t alpha[b][p][t] * Vw[b][t][n]
    h1 = relu((1 + gamma) * Y + conv([lang | grid], W0[:, Cf:]) + bias)
followed by the five remaining convolutions of oracle.zsg_oracle.head_forward.  The concatenated vector `we` (lang_pool's, normalised
under do_norm) still supplies the shift.  With Wv = 0 this is the oracle's head up to the split of conv0's sum.
zsgnet_forward composes the oracle's pieces and tests/langpool_ref.py's query encoder, as tests/film_ref.py does."""
import math

import torch
import torch.nn.functional as F

import langpool_ref as LR
from oracle import zsg_oracle as O


def token_outputs(sd, qvec, qlens, h0, c0, rank=None, bidirectional=True):
    """(o [B, T, D] padded with zeros at t >= len, lens: list of int) — langpool_ref.lstm_outputs as one tensor"""
    if rank is None:
        rank = O.sort_rank(qlens)
    seqs, starts = LR.lstm_outputs(sd, qvec, qlens, h0, c0, rank, bidirectional)
    T, D = qvec.shape[1], starts[0].shape[1]
    rows = []
    for s in seqs:
        pad = [torch.zeros(1, D, dtype=starts[0].dtype)] * (T - len(s))
        rows.append(torch.cat(list(s) + pad, dim=0))
    return torch.stack(rows, dim=0), [len(s) for s in seqs]


def attention(y, Kw, Vw, lens, scale):
    """y [B, N, h, w], Kw / Vw [B, T, N] -> (gamma [B, N, h, w], alpha [B, h*w, T]); the softmax runs over each sample's t < len"""
    B, N, h, w = y.shape
    T = Kw.shape[1]
    rows = y.permute(0, 2, 3, 1).reshape(B, h * w, N)
    gam, alp = [], []
    for b in range(B):
        n = lens[b]
        a = torch.zeros(h * w, T, dtype=y.dtype)
        if n > 0:
            s = scale * (rows[b] @ Kw[b, :n].t())                 # [P, n]
            an = torch.softmax(s - s.max(dim=1, keepdim=True).values.detach(), dim=1)
            a = torch.cat([an, a[:, n:]], dim=1)
        alp.append(a)
        gam.append(a[:, :n] @ Vw[b, :n])                          # [P, N]  (n = 0: zeros)
    gamma = torch.stack(gam, 0).reshape(B, h, w, N).permute(0, 3, 1, 2)
    return gamma, torch.stack(alp, 0)


def words_h1(sd, feat, we, o, lens, prefix="att_reg_box."):
    """(h1 [B, N, h, w], Y, alpha [B, h*w, T]) of one pyramid level"""
    Cf = feat.shape[1]
    W0, b0 = sd[prefix + "0.0.weight"], sd[prefix + "0.0.bias"]
    rest = O.fuse_lang_grid(feat, we)[:, Cf:]                     # [lang | grid] exactly as the concatenation builds them
    y = F.conv2d(feat, W0[:, :Cf], None, 1, 1)
    Kw = o @ sd[prefix + "words.key.weight"].t()                  # [B, T, N]
    Vw = o @ sd[prefix + "words.value.weight"].t()
    gamma, alpha = attention(y, Kw, Vw, lens, 1.0 / math.sqrt(y.shape[1]))
    return F.relu((1 + gamma) * y + F.conv2d(rest, W0[:, Cf:], None, 1, 1) + b0[None, :, None, None]), y, alpha


def words_head(sd, feat, we, o, lens, prefix="att_reg_box.", outc=5):
    """One 6-convolution head on one pyramid level: feat [B, Cf, h, w], we [B, D], o [B, T, D] -> [B, h*w*A, outc]"""
    B = feat.shape[0]
    x = words_h1(sd, feat, we, o, lens, prefix)[0]
    for i in range(1, 5):
        x = F.relu(F.conv2d(x, sd[f"{prefix}{i}.0.weight"], sd[f"{prefix}{i}.0.bias"], 1, 1))
    x = F.conv2d(x, sd[prefix + "5.weight"], sd[prefix + "5.bias"], 1, 1)
    return x.permute(0, 2, 3, 1).contiguous().view(B, -1, outc)


def heads(sd, feats, we, o, lens):
    """(att [B, A, 1], bbx [B, A, 4]) over all levels"""
    if "att_reg_box.5.weight" in sd:
        ab = torch.cat([words_head(sd, f, we, o, lens) for f in feats], dim=1)
        return ab[..., 4:5], ab[..., :4]
    att = torch.cat([words_head(sd, f, we, o, lens, "att_box.", 1) for f in feats], dim=1)
    bbx = torch.cat([words_head(sd, f, we, o, lens, "reg_box.", 4) for f in feats], dim=1)
    return att, bbx


def zsgnet_forward(sd, batch, h0, c0, arch="resnet50", training=True, six_hundred=False, rank=None, do_norm=False, bidirectional=True,
                   lang_pool="final"):
    """oracle.zsg_oracle.zsgnet_forward for the ResNet-FPN trunk with the word-attention head (use_lang and use_img: words needs both).
    The definition holds for every lang_pool, "last" included (the network refuses that one: its program never forms o)."""
    bn = O.BNState(sd, training)
    if rank is None:
        rank = O.sort_rank(batch["qlens"])
    we = LR.query_encoder(sd, batch["qvec"], batch["qlens"], h0, c0, rank, bidirectional, lang_pool)
    o, lens = token_outputs(sd, batch["qvec"], batch["qlens"], h0, c0, rank, bidirectional)
    c3, c4, c5 = O.encoder_forward(sd, batch["img"], arch, bn)
    feats = O.fpn_forward(sd, c3, c4, c5, six_hundred)
    wn = we
    if do_norm:
        feats = [f / f.norm(dim=1, keepdim=True) for f in feats]
        wn = we / we.norm(dim=1, keepdim=True)
    att, bbx = heads(sd, feats, wn, o, lens)
    return dict(att_out=att, bbx_out=bbx, feat_sizes=torch.tensor([[f.shape[2], f.shape[3]] for f in feats]),
                num_f_out=torch.tensor([len(feats)]), we=we, feats=feats, o=o)

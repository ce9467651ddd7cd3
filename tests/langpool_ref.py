"""Host definition of cfg lang_pool (last / final / mean / attn): plain torch, any dtype, differentiable.

All modes share the LSTM weights, the gate order (i, f, g, o: oracle.zsg_oracle.lstm_cell), the h0 / c0 rule (sample b starts from row
rank[b] of its direction's half, rank = stable descending sort of qlens) and the length clamp len = clamp(qlens[b], 0, T) of the `last`
encoder.  With f_t the forward state after x_0..x_t and r_t the reverse state after x_{len-1}, .., x_t, the padded output of
torch.nn.LSTM on the packed batch is o_t = [f_t | r_t], t < len (o_t = f_t with one direction):
    last   we = [f_{len-1} | r_{len-1}]          (oracle.zsg_oracle.query_encoder: the reference's vector)
    final  we = [f_{len-1} | r_0]                (nn.LSTM's h_n)
    mean   we = (1 / len) sum_{t < len} o_t
    attn   s_t = w . o_t,  alpha = softmax over t < len of s,  we = sum_t alpha_t o_t,   w = sd["lang_pool.weight"] [1, D]
A row with len = 0 gives we = 0 for mean / attn and the starting states for last / final.
zsgnet_forward is oracle.zsg_oracle.zsgnet_forward (ResNet-FPN trunk) with this query encoder, assembled from the oracle's public pieces."""
import torch

from oracle import zsg_oracle as O

MODES = ("last", "final", "mean", "attn")


def lstm_outputs(sd, qvec, qlens, h0, c0, rank, bidirectional=True):
    """Per sample the list of o_t [1, D], t < len (empty at len = 0), and the starting states [1, D]"""
    B, T = qvec.shape[0], qvec.shape[1]
    sufs = [""] + (["_reverse"] if bidirectional else [])
    seqs, starts = [], []
    for b in range(B):
        r = int(rank[b])
        n = max(0, min(int(qlens[b]), T))
        per_dir = []
        for di, suf in enumerate(sufs):
            p = [sd[f"lstm.{k}_l0{suf}"] for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
            h, c = h0[di, r:r + 1], c0[di, r:r + 1]
            out = [None] * n
            for t in (range(n) if di == 0 else range(n - 1, -1, -1)):
                h, c = O.lstm_cell(qvec[b:b + 1, t], h, c, *p)
                out[t] = h
            per_dir.append(out)
        seqs.append([torch.cat([o[t] for o in per_dir], dim=1) for t in range(n)])
        starts.append(torch.cat([h0[di, r:r + 1] for di in range(len(sufs))], dim=1))
    return seqs, starts


def pool(seq, start, mode, w=None, H=None):
    """One sample's vector [1, D] from its o_t list"""
    n = len(seq)
    if mode in ("last", "final"):
        if n == 0:
            return start
        if mode == "last" or H is None or seq[0].shape[1] == H:
            return seq[n - 1]
        return torch.cat([seq[n - 1][:, :H], seq[0][:, H:]], dim=1)
    if n == 0:
        return torch.zeros_like(start)
    o = torch.cat(seq, dim=0)                       # [len, D]
    if mode == "mean":
        return o.sum(0, keepdim=True) / n
    s = o @ w.reshape(-1)
    a = torch.softmax(s - s.max().detach(), dim=0)
    return (a.unsqueeze(1) * o).sum(0, keepdim=True)


def query_encoder(sd, qvec, qlens, h0, c0, rank=None, bidirectional=True, mode="last"):
    """we [B, D], D = H x directions"""
    if mode not in MODES:
        raise ValueError(f"lang_pool={mode!r}")
    if rank is None:
        rank = O.sort_rank(qlens)
    H = h0.shape[2]
    seqs, starts = lstm_outputs(sd, qvec, qlens, h0, c0, rank, bidirectional)
    w = sd["lang_pool.weight"] if mode == "attn" else None
    return torch.cat([pool(s, st, mode, w, H) for s, st in zip(seqs, starts)], dim=0)


def zsgnet_forward(sd, batch, h0, c0, arch="resnet50", training=True, six_hundred=False, rank=None, use_lang=True, use_img=True,
                   bidirectional=True, lang_pool="last"):
    """oracle.zsg_oracle.zsgnet_forward for the ResNet-FPN trunk (no do_norm) with `lang_pool`'s sentence vector"""
    bn = O.BNState(sd, training)
    we = query_encoder(sd, batch["qvec"], batch["qlens"], h0, c0, rank, bidirectional, lang_pool)
    c3, c4, c5 = O.encoder_forward(sd, batch["img"], arch, bn)
    feats = O.fpn_forward(sd, c3, c4, c5, six_hundred)
    xs = [O.head_input(f, we, use_lang, use_img) for f in feats]
    if "att_reg_box.5.weight" in sd:
        ab = torch.cat([O.head_forward(sd, x) for x in xs], dim=1)
        att, bbx = ab[..., 4:5], ab[..., :4]
    else:
        att = torch.cat([O.head_forward(sd, x, "att_box.", 1) for x in xs], dim=1)
        bbx = torch.cat([O.head_forward(sd, x, "reg_box.", 4) for x in xs], dim=1)
    return dict(att_out=att, bbx_out=bbx, feat_sizes=torch.tensor([[f.shape[2], f.shape[3]] for f in feats]),
                num_f_out=torch.tensor([len(feats)]), we=we, feats=feats)

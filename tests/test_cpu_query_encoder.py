"""The oracle's query encoder (oracle.zsg_oracle.query_encoder, both directions and the single-direction form) pinned
against torch.nn.LSTM itself, independently of the reference tree: float64 on both sides, nn.LSTM driven the way the
reference's apply_lstm drives it (stable descending sort of the lengths, packed sequence, initial state indexed by sorted
position, unsort, output taken at len - 1).  Only the order of the two bias / matrix-product additions inside a cell
differs between the two, so values and the gradients of every LSTM parameter must agree to 1e-12.
Also: ZSGNet refuses an lstm_dim / emb_dim the HIP kernels cannot run, at construction."""
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from oracle import zsg_oracle as O

NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def nn_lstm_last(lstm, qvec, qlens, h0, c0):
    """[B, nd * H]: nn.LSTM over the length-sorted packed batch, output at each sample's last token, in batch order."""
    T = qvec.shape[1]
    lens, perm = torch.sort(qlens, descending=True, stable=True)
    packed = pack_padded_sequence(qvec[perm].transpose(0, 1).contiguous(), lengths=lens.long(), batch_first=False)
    out, _ = pad_packed_sequence(lstm(packed, (h0, c0))[0], batch_first=False, total_length=T)      # [T, B, nd * H]
    last = out[lens.long() - 1, torch.arange(len(lens))]
    res = torch.zeros_like(last)
    res[perm] = last
    return res


@pytest.mark.parametrize("H,bid,E", [(32, True, 300), (64, False, 300), (256, True, 100), (128, False, 52)])
def test_query_encoder_equals_packed_nn_lstm(H, bid, E):
    B, T, nd = 5, 9, 2 if bid else 1
    g = torch.Generator().manual_seed(H + E)
    qvec = torch.randn(B, T, E, generator=g, dtype=torch.float64) * 0.35
    qlens = torch.tensor([4.0, 9.0, 4.0, 9.0, 1.0])          # ties: the sort must be the stable one
    h0, c0 = torch.randn(nd, B, H, generator=g, dtype=torch.float64), torch.randn(nd, B, H, generator=g, dtype=torch.float64)
    gw = torch.randn(B, nd * H, generator=g, dtype=torch.float64)
    sd = {k: v.double() for k, v in O.seeded_state_dict("resnet18", 3, emb_dim=E, lstm_dim=H).items() if k.startswith("lstm.")}
    sufs = [""] + (["_reverse"] if bid else [])
    if not bid:
        sd = {k: v for k, v in sd.items() if not k.endswith("_reverse")}
    lstm = torch.nn.LSTM(E, H, bidirectional=bid).double()
    assert {n for n, _ in lstm.named_parameters()} == {n + s for n in NAMES for s in sufs}
    with torch.no_grad():
        for n, p in lstm.named_parameters():
            p.copy_(sd["lstm." + n])
    want = nn_lstm_last(lstm, qvec, qlens, h0, c0)
    (want * gw).sum().backward()
    for v in sd.values():
        v.requires_grad_()
    got = O.query_encoder(sd, qvec, qlens, h0, c0, bidirectional=bid)
    (got * gw).sum().backward()
    assert got.shape == (B, nd * H)
    assert float((got - want).detach().abs().max()) <= 1e-12
    for n, p in lstm.named_parameters():
        e = float((sd["lstm." + n].grad - p.grad).abs().max())
        assert e <= 1e-12, f"d {n}: {e:.3g}"
    # the default stays the bidirectional encoder
    if bid:
        assert torch.equal(O.query_encoder(sd, qvec, qlens, h0, c0), got)


@pytest.mark.parametrize("flags,key,values", [(dict(lstm_dim=100), "lstm_dim", ("32", "64", "128", "256")),
                                              (dict(lstm_dim=512), "lstm_dim", ("32", "64", "128", "256")),
                                              (dict(emb_dim=50), "emb_dim", ("multiples of 4",)),
                                              (dict(emb_dim=0), "emb_dim", ("multiples of 4",))])
def test_unsupported_encoder_sizes_are_refused_at_construction(monkeypatch, flags, key, values):
    from zsgnet_pytorch_amd import config, mdl, params
    made = []
    monkeypatch.setattr(params.ParamStore, "allocate", lambda self, *a, **k: made.append(self))      # nothing may get this far
    with pytest.raises(ValueError) as ei:
        mdl.get_default_net(9, config.get_cfg(resnet_arch="resnet18", **flags))
    assert not made, "parameters were allocated before the refusal"
    msg = str(ei.value)
    assert f"{key}={flags[key]}" in msg and all(v in msg for v in values), msg


@pytest.mark.parametrize("flags", [dict(lstm_dim=32), dict(lstm_dim=256, use_bidirectional=False), dict(emb_dim=52)])
def test_supported_encoder_sizes_construct(flags):
    from zsgnet_pytorch_amd import config, mdl
    cfg = config.get_cfg(resnet_arch="resnet18", **flags)
    net = mdl.get_default_net(9, cfg)
    nd = 2 if cfg["use_bidirectional"] else 1
    H, E = cfg["lstm_dim"], cfg["emb_dim"]
    P = dict(net.named_parameters())
    assert P["lstm.weight_ih_l0"].shape == (4 * H, E) and P["lstm.weight_hh_l0"].shape == (4 * H, H)
    assert ("lstm.weight_ih_l0_reverse" in P) == (nd == 2)
    assert P["att_reg_box.0.0.weight"].shape[1] == 256 + nd * H + 2
    h0, c0 = net.lstm_init_hidden(3)
    assert h0.shape == c0.shape == (nd, 3, H)

"""Fine-tuning on the host side (no GPU): the data-parallel reducer's spans skip frozen parameters, FusedAdam accepts torch.optim
parameter groups of the model's own parameters only."""
import pytest
import torch


def _net():
    from zsgnet_pytorch_amd import config, mdl
    return mdl.get_default_net(9, config.get_cfg(resnet_arch="resnet18"))


def test_reducer_spans_skip_frozen_parameters():
    from zsgnet_pytorch_amd.dist import grad_spans, plan_buckets
    net = _net()
    ents, names = net.store.entries, net._param_names
    frozen = {n for n in names if n.startswith("backbone.encoder.")}
    assert frozen and len(frozen) < len(names)
    ready = {n: i for i, n in enumerate(reversed(names))}
    full = grad_spans(ents, names, ready)
    assert full == [(ents[n].offset, (ents[n].size + 3) // 4 * 4, ready[n]) for n in names]
    spans = grad_spans(ents, names, ready, frozen)
    assert [s[0] for s in spans] == [ents[n].offset for n in names if n not in frozen]
    fz = [(ents[n].offset, ents[n].offset + (ents[n].size + 3) // 4 * 4) for n in frozen]
    buckets = plan_buckets(spans, 1 << 20, tail_elems=1 << 16)
    assert sum(b.end - b.start for b in buckets) == sum(s[1] for s in spans)          # the trainable spans, each exactly once
    for b in buckets:
        assert not any(b.start < e and s < b.end for s, e in fz), "a bucket covers a frozen span"
    assert plan_buckets(grad_spans(ents, names, ready, set(names)), 1 << 20, tail_elems=1 << 16) == []


def test_fused_adam_groups_validation():
    from zsgnet_pytorch_amd import optim
    net = _net()
    ps = dict(net.named_parameters())
    enc = [p for n, p in ps.items() if n.startswith("backbone.encoder.")]
    rest = [p for n, p in ps.items() if not n.startswith("backbone.encoder.")]
    opt = optim.FusedAdam(net, lr=1e-3, params=[dict(params=enc, lr=1e-4), dict(params=rest[:5])])
    assert [g["lr"] for g in opt.param_groups] == [1e-4, 1e-3]
    opt.add_param_group(dict(params=rest[5:], weight_decay=0.1))
    assert len(opt.param_groups) == 3 and opt.param_groups[2]["weight_decay"] == 0.1
    with pytest.raises(ValueError, match="not a parameter of the model"):
        optim.FusedAdam(net, params=[torch.nn.Parameter(torch.zeros(4))])
    with pytest.raises(ValueError, match="at most 8"):
        optim.FusedAdam(net, params=[dict(params=[p]) for p in rest[:9]])
    gen = optim.FusedAdam(net, params=[dict(params=net.backbone.encoder.parameters(), lr=1e-5)])          # an iterator as group params
    assert len(gen.param_groups[0]["params"]) == len(enc)
    sub = optim.FusedAdam(net, params=iter(rest))
    assert len(sub.param_groups) == 1 and len(sub.param_groups[0]["params"]) == len(rest)
    # a state saved before per-parameter counters existed (one 'step') gives its count to every parameter
    st = sub.state_dict()
    assert int(st["zsg"]["steps"].numel()) == len(ps)
    del st["zsg"]["steps"]
    st["zsg"]["step"] = torch.tensor([6], dtype=torch.int32)
    sub.load_state_dict(st)
    assert sub.param_steps().tolist() == [6] * len(ps)

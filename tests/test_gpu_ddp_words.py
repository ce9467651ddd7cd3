"""cfg lang_fuse = "words" under the data-parallel wrapper.

TWO RANKS sharing one GPU over gloo (as tests/test_gpu_ddp_finetune.py / _clip.py), each with a batch of its own.  Every rank also runs
the un-wrapped network on BOTH batches; the reduced gradient — each rank's pre-scaled by 1/2 (exact), then one fp32 add — must be
0.5 * g_0 + 0.5 * g_1 of those plain backwards bit for bit, on both ranks.  A bucket handed to the reducer before its last writer has
landed would average a partial value and let the late launch add only the rank's own share on top: the ranks would then differ from the
mean and from each other.  That covers the grad_ready entries of the two words weights and the query encoder's gradients, which under
this mode wait for the heads' deferred d(o) launches replayed behind the pool's backward.  Small buckets (1 MB), so that those tensors
are reduced while the rest of the backward is still running.
Beside it the 1-rank `nccl` group of tests/test_gpu_ddp_film.py with every collective forced (the bucket plan covers the new tensors)."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

KEYS = ("att_reg_box.words.key.weight", "att_reg_box.words.value.weight")


def _worker(port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0", ZSG_DETERMINISTIC="1")
    import torch.distributed as dist
    from oracle import zsg_oracle as O
    from zsgnet_pytorch_amd import config, dist as zdist, loss, mdl, optim
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    cfg = config.get_cfg(resnet_arch="resnet18", lang_fuse="words", lang_pool="mean")
    sd = O.seeded_state_dict("resnet18", 41)
    g = torch.Generator().manual_seed(5)
    for k in KEYS:
        sd[k] = torch.randn(256, 256, generator=g) * 0.05
    r, s = config.ratios_scales(cfg)
    lf = loss.get_default_loss(r, s, cfg)
    bt = {k: v.cuda() for k, v in O.synthetic_batch(2, 96, 96, seed=72).items()}
    bt["h0"], bt["c0"] = torch.zeros(2, 2, 128), torch.zeros(2, 2, 128)
    info = {}

    def run(wrap):
        net = mdl.get_default_net(9, cfg)
        net.load_state_dict(sd)
        net.to("cuda").train()
        model = zdist.DistributedDataParallel(net, device_ids=[0], comm="torch", force_collectives=True, bucket_mb=4.0) if wrap else net
        opt = optim.FusedAdam(net, lr=1e-3)
        opt.zero_grad()
        lf(model(bt), bt)["loss"].backward()
        torch.cuda.synchronize()
        g = net.store.grad.clone().cpu()
        info["spans"] = [(net.store.entries[k].offset, net.store.entries[k].offset + net.store.entries[k].size) for k in KEYS]
        if wrap:
            plan = net._plans[list(net._plans)[0]]
            info["buckets"] = [(b.start, b.end, b.ready) for b in plan.reducer.buckets]
            info["flat"] = int(net.store.grad.numel())
            info["ready"] = [plan.grad_ready.get(k) for k in KEYS]
        opt.step()
        opt.zero_grad()
        ls = lf(model(bt), bt)["loss"]
        ls.backward()                        # second step: reducer reuse
        torch.cuda.synchronize()
        return g, bool(torch.isfinite(ls)) and bool(torch.isfinite(net.store.grad).all())
    g_plain, _ = run(False)
    g_ddp, fin = run(True)
    torch.save(dict(g_plain=g_plain, g_ddp=g_ddp, finite=fin, **info), os.path.join(out_dir, "words.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_reduced_gradients_equal_the_plain_backward(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ctx = mp.get_context("spawn")
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    p = ctx.Process(target=_worker, args=(port, str(tmp_path)))
    p.start()
    p.join(600)
    assert p.exitcode == 0, "the nccl-backend rank failed or hung"
    r = torch.load(tmp_path / "words.pt")
    assert torch.equal(r["g_ddp"], r["g_plain"]), "1-rank reduced gradients must equal the plain backward's"
    (klo, khi), (vlo, vhi) = r["spans"]
    assert float(r["g_ddp"][klo:khi].abs().max()) > 0 and float(r["g_ddp"][vlo:vhi].abs().max()) > 0
    assert khi == vlo and vhi == r["flat"], "key then value, at the end of the flat buffer"
    assert r["finite"] and all(x is not None for x in r["ready"])
    assert sum(e - s for s, e, _ in r["buckets"]) == r["flat"], "the buckets cover the flat gradient buffer once, the new tensors included"


def _worker2(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      ZSG_DETERMINISTIC="1", ZSG_AUTOTUNE="0")      # (no tile choice by timing: both processes run the same launch shapes)
    import torch.distributed as dist
    from oracle import zsg_oracle as O
    from zsgnet_pytorch_amd import config, dist as zdist, loss, mdl, optim
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = config.get_cfg(resnet_arch="resnet18", lang_fuse="words", lang_pool="mean")
    sd = O.seeded_state_dict("resnet18", 41)
    g = torch.Generator().manual_seed(5)
    for k in KEYS:
        sd[k] = torch.randn(256, 256, generator=g) * 0.05
    r, s = config.ratios_scales(cfg)
    lf = loss.get_default_loss(r, s, cfg)

    def batch(rk):
        bt = {k: v.cuda() for k, v in O.synthetic_batch(2, 96, 96, seed=72 + rk).items()}
        bt["h0"], bt["c0"] = torch.zeros(2, 2, 128), torch.zeros(2, 2, 128)
        return bt

    def fresh():
        net = mdl.get_default_net(9, cfg)
        net.load_state_dict(sd)
        return net.to("cuda").train()
    plain = []
    for rk in range(world):                  # the plain backward of either rank's batch, on the starting weights
        net = fresh()
        opt = optim.FusedAdam(net, lr=1e-3)
        opt.zero_grad()
        bt = batch(rk)
        lf(net(bt), bt)["loss"].backward()
        torch.cuda.synchronize()
        plain.append(net.store.grad.clone().cpu())
    net = fresh()
    ddp = zdist.DistributedDataParallel(net, device_ids=[0], broadcast_buffers=True, bucket_mb=1.0)
    opt = optim.FusedAdam(net, lr=1e-3)
    bt = batch(rank)
    reduced = []
    for _ in range(2):                       # (second step: reducer reuse on weights that have moved)
        opt.zero_grad()
        lf(ddp(bt), bt)["loss"].backward()
        torch.cuda.synchronize()
        reduced.append(net.store.grad.clone().cpu())
        opt.step()
    torch.cuda.synchronize()
    plan = net._plans[list(net._plans)[0]]
    ent = net.store.entries
    spans = {k: (ent[k].offset, ent[k].offset + ent[k].size) for k in KEYS + ("lstm.weight_hh_l0", "lstm.weight_ih_l0_reverse")}
    torch.save(dict(plain=plain, reduced=reduced, spans=spans, buckets=[(b.start, b.end, b.ready) for b in plan.reducer.buckets],
                    flat=int(net.store.grad.numel()), ready={k: plan.grad_ready.get(k) for k in spans}, nbwd=len(plan.bwd.calls)),
               os.path.join(out_dir, f"r{rank}.pt"))
    ddp.close()
    dist.destroy_process_group()


def test_two_ranks_reduce_to_the_mean_of_the_plain_backwards(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker2, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
        assert p.exitcode == 0, "a rank failed or hung"
    res = [torch.load(tmp_path / f"r{r}.pt") for r in range(2)]
    i32 = lambda t: t.view(torch.int32)
    assert all(torch.equal(i32(res[0]["plain"][k]), i32(res[1]["plain"][k])) for k in range(2)), "the plain backward is the same on either rank"
    g0, g1 = res[0]["plain"]
    assert not torch.equal(g0, g1)
    want = g0 * 0.5 + g1 * 0.5
    for r in res:
        assert len(r["buckets"]) > 4 and sum(e - s for s, e, _ in r["buckets"]) == r["flat"]
        got = r["reduced"][0]
        for k, (lo, hi) in r["spans"].items():
            assert float(want[lo:hi].abs().max()) > 0 and not torch.equal(g0[lo:hi], g1[lo:hi]), k
            assert torch.equal(got[lo:hi] + 0, want[lo:hi] + 0), f"{k}: reduced before its last writer had landed?"
        assert torch.equal(got + 0, want + 0), "the reduced gradient is not the mean of the two plain backwards"
        assert bool(torch.isfinite(r["reduced"][1]).all())
        # every tensor this mode adds or re-orders has a readiness index, and its bucket is released no earlier than that
        for k, (lo, hi) in r["spans"].items():
            rd = r["ready"][k]
            assert rd is not None and 0 < rd <= r["nbwd"], k
            mine = [b for b in r["buckets"] if b[0] < hi and b[1] > lo]
            assert mine and all(b[2] >= rd for b in mine), (k, rd, mine)
    for it in range(2):
        assert torch.equal(i32(res[0]["reduced"][it]), i32(res[1]["reduced"][it])), f"step {it}: the ranks hold different reduced gradients"

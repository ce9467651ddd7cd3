"""wgrad_dtype = "bf16" under the data-parallel wrapper, in one child process with a 1-rank `nccl` group and every collective forced (as
tests/test_gpu_ddp_shared_train.py): the gradients stay fp32, so nothing changes for the reducer — its reduced gradients are bit-equal
to the single-process bf16 plan's (a 1-rank sum, pre-scale 1/1), and the plan's grad_ready (the launch after which a parameter's
gradient may join its bucket) covers every trainable parameter with a valid launch index."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

ENC = "backbone.encoder.layer1."


def _worker(port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0", ZSG_DETERMINISTIC="1")
    import torch.distributed as dist
    from oracle import zsg_oracle as O
    from zsgnet_pytorch_amd import config, dist as zdist, loss, mdl, optim
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    cfg = config.get_cfg(resnet_arch="resnet18", wgrad_dtype="bf16")
    sd = O.seeded_state_dict("resnet18", 40)
    r, s = config.ratios_scales(cfg)
    lf = loss.get_default_loss(r, s, cfg)
    bt = {k: v.cuda() for k, v in O.synthetic_batch(2, 96, 96, seed=70).items()}
    bt["h0"], bt["c0"] = torch.zeros(2, 2, 128), torch.zeros(2, 2, 128)

    def run(wrap):
        net = mdl.get_default_net(9, cfg)
        net.load_state_dict(sd)
        net.to("cuda").train()
        for n, p in net.named_parameters():                  # (a frozen stage: grad_ready must cover the trainable set, not more)
            p.requires_grad_(not n.startswith(ENC))
        model = zdist.DistributedDataParallel(net, device_ids=[0], comm="torch", force_collectives=True, bucket_mb=1.0) if wrap else net
        if wrap:
            assert model.wgrad_precision("bf16") is model and net._wgrad_dtype == "bf16"
        opt = optim.FusedAdam(net, lr=1e-3)
        opt.zero_grad()
        lf(model(bt), bt)["loss"].backward()
        torch.cuda.synchronize()
        g = net.store.grad.clone().cpu()
        plan = [p for k, p in net._plans.items() if k[-1]][0]
        names = [fn.__name__ for fn, _, _ in plan.bwd.calls]
        info = dict(g=g, n_bf16=names.count("zsg_conv_wgrad_bf16"), n_calls=len(names), ready=dict(plan.grad_ready),
                    trainable=[n for n, p in net.named_parameters() if p.requires_grad],
                    nb=len(plan.reducer.buckets) if wrap else 0,
                    covered=[(b.start, b.end) for b in plan.reducer.buckets] if wrap else [],
                    spans={n: (net.store.entries[n].offset, net.store.entries[n].size) for n in net._param_names})
        opt.step()
        opt.zero_grad()
        ls = lf(model(bt), bt)["loss"]
        ls.backward()                                        # second step: reducer reuse
        torch.cuda.synchronize()
        info["finite"] = bool(torch.isfinite(ls)) and bool(torch.isfinite(net.store.grad).all())
        return info
    res = dict(plain=run(False), ddp=run(True))
    torch.save(res, os.path.join(out_dir, "wgrad_bf16_ddp.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_ddp_wrapper_bf16_weight_gradients_nccl_world1(tmp_path):
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
    r = torch.load(tmp_path / "wgrad_bf16_ddp.pt")
    a, b = r["plain"], r["ddp"]
    assert a["n_bf16"] >= 20 and a["n_bf16"] == b["n_bf16"]
    assert b["nb"] >= 1 and a["finite"] and b["finite"]
    assert float(a["g"].abs().max()) > 0
    assert torch.equal(a["g"], b["g"]), "1-rank reduced gradients must equal the single-process bf16 plan's"
    for info in (a, b):
        assert set(info["trainable"]) <= set(info["ready"]), "grad_ready misses a trainable parameter"
        assert not any(n.startswith(ENC) for n in info["ready"])
        assert all(0 <= info["ready"][n] < info["n_calls"] for n in info["trainable"])
    for n in b["trainable"]:                                 # every trainable parameter lies inside some bucket
        o, sz = b["spans"][n]
        assert any(s <= o and o + sz <= e for s, e in b["covered"]), n


def _worker2(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      ZSG_DETERMINISTIC="1")
    import torch.distributed as dist
    from oracle import zsg_oracle as O
    from zsgnet_pytorch_amd import config, dist as zdist, loss, mdl, ops, optim
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = config.get_cfg(resnet_arch="resnet18")
    net = mdl.get_default_net(9, cfg)
    net.load_state_dict(O.seeded_state_dict("resnet18", 40))
    net.to("cuda").train()
    r, s = config.ratios_scales(cfg)
    lf = loss.get_default_loss(r, s, cfg)
    bt = {k: v.cuda() for k, v in O.synthetic_batch(2, 96, 96, seed=70 + rank).items()}
    bt["h0"], bt["c0"] = torch.zeros(2, 2, 128), torch.zeros(2, 2, 128)
    ddp = zdist.DistributedDataParallel(net, device_ids=[0], bucket_mb=1.0)
    opt = optim.FusedAdam(net, lr=1e-3)

    def step():
        opt.zero_grad()
        lf(ddp(bt), bt)["loss"].backward()
        torch.cuda.synchronize()
        return net.store.grad.clone().cpu()
    g32 = step()                                             # the fp32 plan: tuned by rank 0, broadcast
    tuned_before = ops.TUNE_INFO["tuned_now"]
    ddp.wgrad_precision("bf16")                              # same geometry, new precision: its entries must be exchanged again
    g16 = step()
    mine = {str(k): v for k, v in ops._TUNE_CACHE.items() if "zsg_conv_wgrad_bf16" in str(k)}
    torch.save(dict(g32=g32, g16=g16, bf16_entries=mine, tuned_in_bf16_step=ops.TUNE_INFO["tuned_now"] - tuned_before),
               os.path.join(out_dir, f"w{rank}.pt"))
    ddp.close()
    dist.destroy_process_group()


def test_two_ranks_exchange_the_bf16_tuner_entries_after_a_switch(tmp_path):
    """world = 2 over gloo on one GPU (as tests/test_gpu_ddp_finetune.py): switching the precision on a geometry whose fp32 plan was
    already tuned and broadcast makes rank 0 tune the bf16 entries and broadcast them — rank 1 tunes nothing itself and lowers the same
    tiles, and both ranks end with the same reduced gradient."""
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
    a, b = torch.load(tmp_path / "w0.pt"), torch.load(tmp_path / "w1.pt")
    assert len(a["bf16_entries"]) >= 10 and a["bf16_entries"] == b["bf16_entries"]
    assert b["tuned_in_bf16_step"] == 0, "rank 1 tuned bf16 entries itself: they were not broadcast"
    assert torch.equal(a["g16"], b["g16"]) and torch.equal(a["g32"], b["g32"])
    assert not torch.equal(a["g16"], a["g32"])

"""enc_bwd_dtype = "bf16" under the data-parallel wrapper: two ranks share ONE GPU over gloo (as tests/test_gpu_ddp_enc_bf16.py), ResNet-18
at 96 px, two images per rank, ZSG_DETERMINISTIC=1, with and without synchronized BatchNorm.  Activations and gradients stay fp32 in
memory, so nothing changes for the reducer: the ranks end a step with identical gradients and, after one optimizer step, with bit-equal
weights; the wrapper's encoder_backward_precision reaches the network and the plan key; with synchronized BatchNorm the backward sums of
every BatchNorm whose dout a covered data gradient completes come from that bf16 launch's partial rows (plan.sync_bn_paths[...] ends
with "/bnb" or "/bnb+alias").  Every process group has a timeout and the children are joined with a time limit."""
import datetime
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

ENC = "backbone.encoder."


def _worker(rank, world, port, out_dir, sync):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      ZSG_DETERMINISTIC="1")
    import torch.distributed as dist
    from oracle import zsg_oracle as O
    from zsgnet_pytorch_amd import config, dist as zdist, loss, mdl, optim
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=240))
    cfg = config.get_cfg(resnet_arch="resnet18")
    net = mdl.get_default_net(9, cfg)
    net.load_state_dict(O.seeded_state_dict("resnet18", 17))
    net.to("cuda").train()
    r, s = config.ratios_scales(cfg)
    lf = loss.get_default_loss(r, s, cfg)
    model = zdist.DistributedDataParallel(net, device_ids=[0], broadcast_buffers=True, bucket_mb=1.0)
    if sync:
        assert zdist.convert_sync_batchnorm(model) is model
    assert model.encoder_backward_precision("bf16") is model and net._enc_bwd_dtype == "bf16" and net._enc_dtype == "fp32"
    opt = optim.FusedAdam(net, lr=1e-4, betas=(0.9, 0.99))
    full = O.synthetic_batch(4, 96, 96, seed=70)
    bt = {k: v[2 * rank:2 * rank + 2].cuda() for k, v in full.items()}
    bt["h0"], bt["c0"] = torch.zeros(2, 2, 128), torch.zeros(2, 2, 128)
    opt.zero_grad()
    ls = lf(model(bt), bt)["loss"].mean()
    ls.backward()
    torch.cuda.synchronize()
    grad = net.store.grad.cpu().clone()
    opt.step()
    torch.cuda.synchronize()
    (key,) = [k for k in net._plans if k[-1]]
    plan = net._plans[key]
    log = [e for e in plan._b16_log if e["kind"] == "enc_dgrad"]
    res = dict(grad=grad, weights=net.store.flat.cpu().clone(), loss=float(ls), key_has=key[-2] == ("encb", "bf16"),
               kinds=sorted({e["kind"] for e in plan._b16_log}),
               fns=[plan.bwd.calls[e["idx"]][0].__name__ for e in log], whats=[plan.bwd.calls[e["idx"]][2] for e in log],
               bns=[e["bn"] for e in log], paths=dict(plan.sync_bn_paths), synced=sorted(plan.sync_bn))
    torch.save(res, os.path.join(out_dir, f"r{rank}.pt"))
    model.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("sync", [False, True], ids=["per_rank_bn", "sync_bn"])
def test_two_ranks_end_a_step_with_bit_equal_weights(tmp_path, sync):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path), sync)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(420)
    for p in procs:
        if p.is_alive():
            p.kill()
    assert all(p.exitcode == 0 for p in procs), f"a process failed or hung: {[p.exitcode for p in procs]}"
    r0, r1 = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt")
    for r in (r0, r1):
        assert r["key_has"] and r["kinds"] == ["enc_dgrad"]
        assert len(r["fns"]) == 19 and set(r["fns"]) == {"zsg_conv_igemm_bf16_bnb", "zsg_conv_igemm_bf16_m"}       # ResNet-18: 16 block convolutions + 3 projections
        assert all(w.startswith("dgrad:" + ENC) and (w.endswith("+bf16") or w.endswith("+bf16+bnb")) for w in r["whats"])
        assert all((f == "zsg_conv_igemm_bf16_bnb") == (b is not None) for f, b in zip(r["fns"], r["bns"]))
        assert sum(b is not None for b in r["bns"]) >= 8 and all(b.startswith(ENC) for b in r["bns"] if b is not None)
        assert bool(torch.isfinite(r["grad"]).all()) and float(r["grad"].abs().max()) > 0 and r["loss"] == r["loss"]
    assert torch.equal(r0["grad"].view(torch.int32), r1["grad"].view(torch.int32)), "the ranks' reduced gradients differ"
    assert torch.equal(r0["weights"].view(torch.int32), r1["weights"].view(torch.int32)), "the ranks' weights differ after the step"
    if sync:
        for r in (r0, r1):
            covered = [b for b in r["bns"] if b is not None]
            assert set(covered) <= set(r["synced"])
            for b in covered:
                assert r["paths"][b].split("/")[1] in ("bnb", "bnb+alias"), (b, r["paths"][b])
    else:
        assert not r0["synced"] and not r0["paths"]

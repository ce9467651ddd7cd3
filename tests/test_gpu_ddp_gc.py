"""cfg head_ctx = "gc" under the data-parallel wrapper: the 1-rank `nccl` group of tests/test_gpu_ddp_film.py with every collective forced.
The reduced gradients (a 1-rank sum, pre-scale 1/1) must equal the un-wrapped network's bit for bit, the seven gc tensors' included, and
the bucket plan must cover the new parameters."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

GC_SHAPES = {"key.weight": (1, 256), "fc1.weight": (64, 256), "fc1.bias": (64,), "ln.weight": (64,), "ln.bias": (64,), "fc2.weight": (256, 64),
             "fc2.bias": (256,)}


def _worker(port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0", ZSG_DETERMINISTIC="1")
    import torch.distributed as dist
    from oracle import zsg_oracle as O
    from zsgnet_pytorch_amd import config, dist as zdist, loss, mdl, optim
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    cfg = config.get_cfg(resnet_arch="resnet18", head_ctx="gc")
    sd = O.seeded_state_dict("resnet18", 41)
    g = torch.Generator().manual_seed(5)
    for n, shp in GC_SHAPES.items():
        sd["att_reg_box.gc." + n] = torch.randn(*shp, generator=g) * 0.1 + (1.0 if n == "ln.weight" else 0.0)
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
        info["gc"] = {n: (net.store.entries["att_reg_box.gc." + n].offset, net.store.entries["att_reg_box.gc." + n].size) for n in GC_SHAPES}
        if wrap:
            plan = net._plans[list(net._plans)[0]]
            info["buckets"] = [(b.start, b.end, b.ready) for b in plan.reducer.buckets]
            info["flat"] = int(net.store.grad.numel())
            info["ready"] = [plan.grad_ready.get("att_reg_box.gc." + n) for n in GC_SHAPES]
        opt.step()
        opt.zero_grad()
        ls = lf(model(bt), bt)["loss"]
        ls.backward()                        # second step: reducer reuse
        torch.cuda.synchronize()
        return g, bool(torch.isfinite(ls)) and bool(torch.isfinite(net.store.grad).all())
    g_plain, _ = run(False)
    g_ddp, fin = run(True)
    torch.save(dict(g_plain=g_plain, g_ddp=g_ddp, finite=fin, **info), os.path.join(out_dir, "gc.pt"))
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
    r = torch.load(tmp_path / "gc.pt")
    assert torch.equal(r["g_ddp"], r["g_plain"]), "1-rank reduced gradients must equal the plain backward's"
    end = 0
    for n, (off, size) in r["gc"].items():
        assert float(r["g_ddp"][off:off + size].abs().max()) > 0, n + ": no gradient"
        end = max(end, off + size)
    assert end == r["flat"], "the seven tensors sit at the end of the flat buffer"
    assert r["finite"] and all(x is not None for x in r["ready"])
    assert sum(e - s for s, e, _ in r["buckets"]) == r["flat"], "the buckets cover the flat gradient buffer once, the new tensors included"

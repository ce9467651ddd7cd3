"""Shared-image training under the data-parallel wrapper, in one child process with a 1-rank `nccl` group and every collective forced
(as tests/test_gpu_ddp.py::test_ddp_wrapper_on_the_nccl_backend_world1): the wrapper's gradients for a shared training batch are
bit-equal to the unwrapped shared backward's (a 1-rank sum, pre-scale 1/1), and sync_batchnorm(force=True) together with a shared
training batch raises a RuntimeError that names both."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _worker(port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0", ZSG_DETERMINISTIC="1")
    import torch.distributed as dist
    from oracle import zsg_oracle as O
    from zsgnet_pytorch_amd import config, dist as zdist, loss, mdl, optim, synth
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    cfg = config.get_cfg(resnet_arch="resnet18")
    sd = O.seeded_state_dict("resnet18", 41)
    r, s = config.ratios_scales(cfg)
    lf = loss.get_default_loss(r, s, cfg)
    bt = synth.synthetic_shared_batch(2, 6, 96, 96, seed=72)
    bt["img_idx"] = torch.tensor([1, 0, 0, 1, 1, 0])
    bt = {k: v.cuda() for k, v in bt.items()}
    bt["h0"], bt["c0"] = torch.zeros(2, 6, 128), torch.zeros(2, 6, 128)

    def run(wrap):
        net = mdl.get_default_net(9, cfg)
        net.load_state_dict(sd)
        net.to("cuda").train()
        net.shared_training(True)
        model = zdist.DistributedDataParallel(net, device_ids=[0], comm="torch", force_collectives=True, bucket_mb=4.0) if wrap else net
        opt = optim.FusedAdam(net, lr=1e-3)
        opt.zero_grad()
        lf(model(bt), bt)["loss"].backward()
        torch.cuda.synchronize()
        g = net.store.grad.clone().cpu()
        plans = [p for k, p in net._plans.items() if len(k) == 9]
        nb = len(plans[0].reducer.buckets) if wrap else 0
        opt.step()
        opt.zero_grad()
        ls = lf(model(bt), bt)["loss"]
        ls.backward()                        # second step: reducer reuse
        torch.cuda.synchronize()
        return g, nb, bool(torch.isfinite(ls)) and bool(torch.isfinite(net.store.grad).all()), model, net
    g_plain, _, _, _, _ = run(False)
    g_ddp, nb, fin, model, net = run(True)
    # sync_batchnorm + shared training: refused, naming both, before any collective of that forward
    net.sync_batchnorm(force=True)
    msg = ""
    try:
        model(bt)
    except RuntimeError as e:
        msg = str(e)
    net.sync_batchnorm(enable=False)
    ok_after = bool(torch.isfinite(model(bt)["att_bbx_out"]).all())
    torch.save(dict(g_plain=g_plain, g_ddp=g_ddp, nb=nb, finite=fin, msg=msg, ok_after=ok_after), os.path.join(out_dir, "shared_ddp.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_ddp_wrapper_shared_training_batch_nccl_world1(tmp_path):
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
    r = torch.load(tmp_path / "shared_ddp.pt")
    assert r["nb"] >= 1 and r["finite"]
    assert float(r["g_plain"].abs().max()) > 0
    assert torch.equal(r["g_ddp"], r["g_plain"]), "1-rank reduced gradients must equal the unwrapped shared backward's"
    assert "sync_batchnorm" in r["msg"] and "shared_training" in r["msg"], r["msg"]
    assert r["ok_after"]

"""eval_tta = "flip" under the data-parallel wrapper, in one child process with a 1-rank `nccl` group and every collective forced (as
tests/test_gpu_ddp_wgrad_bf16.py): the wrapper passes the switch through, a validation batch through the wrapper gives the unwrapped
network's TTA output bit for bit (eval plans are per rank: nothing is communicated), the tuner exchange keys and lowers the 2B-row plan
the forward really uses, and a training step through the wrapper is the plain one."""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _worker(port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0", ZSG_DETERMINISTIC="1", ZSG_AUTOTUNE="0")
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch.distributed as dist
    import tta_ref as R
    from oracle import zsg_oracle as O
    from zsgnet_pytorch_amd import config, dist as zdist, loss, mdl, optim
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    cfg = config.get_cfg(resnet_arch="resnet18")
    sd = O.seeded_state_dict("resnet18", 40)
    r, s = config.ratios_scales(cfg)
    lf = loss.get_default_loss(r, s, cfg)
    host = O.synthetic_batch(2, 96, 96, seed=70)
    g = torch.Generator().manual_seed(2)
    host["qvec_flip"] = torch.randn(host["qvec"].shape, generator=g) * 0.35
    h0, c0 = torch.randn(2, 2, 128, generator=g), torch.randn(2, 2, 128, generator=g)
    bt = {k: v.cuda() for k, v in host.items()}
    bt["h0"], bt["c0"] = h0, c0

    def run(wrap):
        net = mdl.get_default_net(9, cfg)
        net.load_state_dict(sd)
        net.to("cuda")
        model = zdist.DistributedDataParallel(net, device_ids=[0], comm="torch", force_collectives=True, bucket_mb=1.0) if wrap else net
        info = {}
        if wrap:
            info["passthrough"] = model.eval_tta("flip") is model and net._eval_tta == "flip"
            try:
                model.eval_tta("vflip")
                info["refused"] = False
            except ValueError:
                info["refused"] = True
        else:
            net.eval_tta("flip")
        model.eval()
        with torch.no_grad():
            out = model(bt)
            if wrap:
                model._sync_tuning(bt)               # (world 1: forward skips it; the exchange itself, on the geometry of this batch)
                info["tuned"] = sorted(model._tuned)
            info["val_loss"] = float(lf(out, bt)["loss"])
        torch.cuda.synchronize()
        info["o"] = out["att_bbx_out"].detach().cpu().clone()
        info["sizes"] = [tuple(v) for v in out["feat_sizes"].tolist()]
        info["eval_keys"] = [k for k in net._plans if not k[-1]]
        if not wrap:
            # the definition, on the unwrapped net: merge_ref of the plain forward of the hand-built 2B rows (before the
            # training forward below moves the BatchNorm running statistics)
            b2, h2, c2 = R.tta_batch(host, h0, c0)
            i2 = {k: v.cuda() for k, v in b2.items()}
            i2["h0"], i2["c0"] = h2, c2
            net.eval().eval_tta("none")
            with torch.no_grad():
                x2 = net(i2)["att_bbx_out"].detach().cpu().numpy()
            info["want"] = torch.from_numpy(R.merge_ref(x2, info["sizes"], 9))
            net.eval_tta("flip")
        model.train()
        opt = optim.FusedAdam(net, lr=1e-3)
        opt.zero_grad()
        lf(model(bt), bt)["loss"].backward()
        torch.cuda.synchronize()
        info["g"] = net.store.grad.clone().cpu()
        info["train_keys"] = [k[:4] for k in net._plans if k[-1]]
        return info
    res = dict(plain=run(False), ddp=run(True))
    torch.save(res, os.path.join(out_dir, "tta_ddp.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_ddp_wrapper_flip_tta_nccl_world1(tmp_path):
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
    r = torch.load(tmp_path / "tta_ddp.pt")
    a, b = r["plain"], r["ddp"]
    assert b["passthrough"] and b["refused"]
    assert tuple(a["o"].shape)[0] == 2 and tuple(b["o"].shape) == tuple(a["o"].shape)
    assert torch.equal(a["o"].view(torch.int32), a["want"].view(torch.int32)), "the unwrapped TTA forward is merge_ref of its 2B rows"
    assert torch.equal(a["o"].view(torch.int32), b["o"].view(torch.int32)), "the wrapped validation batch gives the unwrapped output's bits"
    assert a["val_loss"] == b["val_loss"]
    assert a["eval_keys"] == b["eval_keys"] == [(4, 96, 96, 20, False)]
    assert b["tuned"] == [(4, 96, 96, False)], "the tuner exchange is keyed on the 2B-row geometry"
    assert a["train_keys"] == b["train_keys"] == [(2, 96, 96, 20)] and float(a["g"].abs().max()) > 0
    assert torch.equal(a["g"], b["g"]), "training through the wrapper ignores the switch"

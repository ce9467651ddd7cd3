"""Synchronized BatchNorm in a 1-rank nccl group (a child process): unforced, the conversion changes nothing — the forward and backward
launch lists are the unconverted plan's, as torch's SyncBatchNorm falls back to batch_norm at world size 1; forced, every train-mode layer
goes through the sums -> all-reduce -> finalize / apply chain (stream-ordered RCCL collectives, one per layer and direction) and matches
the plain plan to fp32 summation order; two forced runs are bit-identical under ZSG_DETERMINISTIC=1; eval forwards are untouched."""
import datetime
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _worker(port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", ZSG_DETERMINISTIC="1")
    import torch.distributed as dist
    from oracle import zsg_oracle as O
    from zsgnet_pytorch_amd import config, dist as zdist, mdl
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, timeout=datetime.timedelta(seconds=180))
    net = mdl.get_default_net(9, config.get_cfg(resnet_arch="resnet18"))
    sd = O.seeded_state_dict("resnet18", 3)
    net.load_state_dict(sd)
    net.to("cuda")
    bt = {k: v.cuda() for k, v in O.synthetic_batch(2, 96, 96, seed=4).items()}
    bt["h0"], bt["c0"] = torch.zeros(2, 2, 128), torch.zeros(2, 2, 128)

    def step():
        net.load_state_dict(sd)
        net.train()
        net.store.grad.zero_()
        out = net(bt)["att_bbx_out"]
        (out * torch.linspace(-1, 1, out.numel(), device="cuda").view_as(out)).sum().backward()
        torch.cuda.synchronize()
        plan = [p for k, p in net._plans.items() if k[-1]][0]
        return dict(out=out.detach().cpu(), grad=net.store.grad.cpu().clone(), rmv=net._rmv.cpu().clone(),
                    fwd=[c[2] for c in plan.fwd.calls], bwd=[c[2] for c in plan.bwd.calls], paths=dict(plan.sync_bn_paths),
                    hosts=(sum(c[0].__name__ == "host" for c in plan.fwd.calls), sum(c[0].__name__ == "host" for c in plan.bwd.calls)),
                    nbn=len(plan.sync_bn))

    def evaluate():
        net.load_state_dict(sd)
        net.eval()
        with torch.no_grad():
            o = net(bt)["att_bbx_out"].cpu()
        return o

    res = dict(plain=step(), eval_plain=evaluate())
    zdist.convert_sync_batchnorm(net)                    # world size 1, not forced: per-rank statistics, the same plan
    res["unforced"] = step()
    zdist.convert_sync_batchnorm(net, force=True)
    res["forced"], res["forced2"] = step(), step()
    res["eval_forced"] = evaluate()
    res["n_bn"] = len(net.bns)
    torch.save(res, os.path.join(out_dir, "nccl.pt"))
    dist.destroy_process_group()


def test_one_rank_nccl(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    p = mp.get_context("spawn").Process(target=_worker, args=(port, str(tmp_path)))
    p.start()
    p.join(420)
    if p.is_alive():
        p.kill()
    assert p.exitcode == 0, f"the child failed or hung ({p.exitcode})"
    r = torch.load(tmp_path / "nccl.pt")
    plain, unf, fo, fo2 = r["plain"], r["unforced"], r["forced"], r["forced2"]
    assert unf["fwd"] == plain["fwd"] and unf["bwd"] == plain["bwd"] and unf["hosts"] == (0, 0) and unf["nbn"] == 0
    assert torch.equal(unf["out"], plain["out"]) and torch.equal(unf["grad"], plain["grad"])
    assert fo["nbn"] == r["n_bn"] and fo["hosts"] == (r["n_bn"], r["n_bn"])   # one collective per layer and direction
    assert fo["fwd"] != plain["fwd"] and all("/" in v for v in fo["paths"].values()), fo["paths"]
    rel = lambda a, b: float((a.double() - b.double()).abs().max()) / (float(b.double().abs().max()) + 1e-30)  # noqa: E731
    assert rel(fo["out"], plain["out"]) < 1e-3, rel(fo["out"], plain["out"])
    assert rel(fo["grad"], plain["grad"]) < 2e-3, rel(fo["grad"], plain["grad"])
    assert float(((fo["rmv"] - plain["rmv"]).abs() / (plain["rmv"].abs() + 1e-3)).max()) < 1e-4
    for k in ("out", "grad", "rmv"):
        assert torch.equal(fo[k], fo2[k]), k                   # bit-reproducible
    assert torch.equal(r["eval_forced"], r["eval_plain"])     # eval forwards are not synced

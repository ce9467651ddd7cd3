"""train_dtype = "bf16_head" under the data-parallel wrapper, in one child process with a 1-rank `nccl` group and every collective forced (as
tests/test_gpu_ddp_wgrad_bf16.py): activations and gradients stay fp32 in memory, so nothing changes for the reducer — its reduced
gradients are bit-equal to the single-process bf16_head plan's (a 1-rank sum, pre-scale 1/1), the plan's grad_ready covers the trainable
set with valid launch indices, and a second step reuses the reducer."""
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
    cfg = config.get_cfg(resnet_arch="resnet18")
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
        assert model.train_precision("bf16_head") is model and net._train_dtype == "bf16_head"      # (the wrapper's, or the net's own)
        opt = optim.FusedAdam(net, lr=1e-3)
        opt.zero_grad()
        lf(model(bt), bt)["loss"].backward()
        torch.cuda.synchronize()
        g = net.store.grad.clone().cpu()
        (key,) = [k for k in net._plans if k[-1]]
        plan = net._plans[key]
        fnames = [fn.__name__ for fn, _, _ in plan.fwd.calls]
        bnames = [fn.__name__ for fn, _, _ in plan.bwd.calls]
        reducer = plan.reducer
        info = dict(g=g, key_has=("train", "bf16_head") in key, n_fwd=fnames.count("zsg_conv_igemm_bf16"), n_dgrad=bnames.count("zsg_conv_igemm_bf16_m"),
                    n_calls=len(bnames), ready=dict(plan.grad_ready), trainable=[n for n, p in net.named_parameters() if p.requires_grad],
                    nb=len(reducer.buckets) if wrap else 0, covered=[(b.start, b.end) for b in reducer.buckets] if wrap else [],
                    spans={n: (net.store.entries[n].offset, net.store.entries[n].size) for n in net._param_names})
        opt.step()
        opt.zero_grad()
        ls = lf(model(bt), bt)["loss"]
        ls.backward()                                        # second step: reducer reuse
        torch.cuda.synchronize()
        info["finite"] = bool(torch.isfinite(ls)) and bool(torch.isfinite(net.store.grad).all())
        info["g2"] = net.store.grad.clone().cpu()
        info["same_reducer"] = plan.reducer is reducer and [k for k in net._plans if k[-1]] == [key]
        return info
    res = dict(plain=run(False), ddp=run(True))
    torch.save(res, os.path.join(out_dir, "train_bf16_head_ddp.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_ddp_wrapper_bf16_head_nccl_world1(tmp_path):
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
    r = torch.load(tmp_path / "train_bf16_head_ddp.pt")
    a, b = r["plain"], r["ddp"]
    assert a["key_has"] and b["key_has"]
    assert a["n_fwd"] >= 10 and a["n_fwd"] == b["n_fwd"] and a["n_dgrad"] >= 8 and a["n_dgrad"] == b["n_dgrad"]
    assert b["nb"] >= 1 and a["finite"] and b["finite"] and a["same_reducer"] and b["same_reducer"]
    assert float(a["g"].abs().max()) > 0
    assert torch.equal(a["g"], b["g"]), "1-rank reduced gradients must equal the single-process bf16_head plan's"
    assert torch.equal(a["g2"], b["g2"]), "... and so must the second step's (fresh packed weights behind the optimizer step, reducer reuse)"
    for info in (a, b):
        assert set(info["trainable"]) <= set(info["ready"]), "grad_ready misses a trainable parameter"
        assert not any(n.startswith(ENC) for n in info["ready"])
        assert all(0 <= info["ready"][n] < info["n_calls"] for n in info["trainable"])
    for n in b["trainable"]:                                 # every trainable parameter lies inside some bucket
        o, sz = b["spans"][n]
        assert any(s <= o and o + sz <= e for s, e in b["covered"]), n

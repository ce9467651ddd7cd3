"""ema.ModelEma on the network (Weight EMA): attached to FusedAdam over real training steps it follows the fp64 recurrence
of tests/ema_ref.py within the trajectory bound and leaves the training itself bit for bit alone; it keeps averaging a parameter that was
frozen on the way (the segmented path); applied() turns the network into the averaged model and restores everything; Learner trains,
validates, checkpoints and resumes with it.  ResNet-18, 96 px, B = 2 (as test_gpu_clip_net.py), ZSG_DETERMINISTIC=1."""
import os

import pytest
import torch

import ema_ref

pytestmark = pytest.mark.gpu

from oracle import zsg_oracle as O  # noqa: E402

ENC = "backbone.encoder."


@pytest.fixture(scope="module")
def Z():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib, config, ema, loss, mdl, optim
    return _lib, config, ema, loss, mdl, optim


@pytest.fixture(autouse=True)
def deterministic(Z):
    """ZSG_DETERMINISTIC=1 for the plans lowered inside and the library's reductions (two runs on the same seeds give the same bits)"""
    L = Z[0]
    old = os.environ.get("ZSG_DETERMINISTIC")
    os.environ["ZSG_DETERMINISTIC"] = "1"
    L.lib.zsg_set_deterministic(1)
    yield
    if old is None:
        os.environ.pop("ZSG_DETERMINISTIC", None)
    else:
        os.environ["ZSG_DETERMINISTIC"] = old
    L.lib.zsg_set_deterministic(1 if old == "1" else 0)


def build(Z, seed=31):
    _lib, config, ema, loss, mdl, optim = Z
    cfg = config.get_cfg(resnet_arch="resnet18")
    net = mdl.get_default_net(9, cfg)
    net.load_state_dict(O.seeded_state_dict("resnet18", seed))
    net.to("cuda").train()
    r, s = config.ratios_scales(cfg)
    return net, loss.get_default_loss(r, s, cfg)


def batch(B=2, hw=96, seed=5):
    bt = O.synthetic_batch(B, hw, hw + 32, seed=seed, tmax=13)
    gq = torch.Generator().manual_seed(2)
    inp = {k: v.cuda() for k, v in bt.items()}
    inp["h0"], inp["c0"] = torch.randn(2, B, 128, generator=gq), torch.randn(2, B, 128, generator=gq)
    return inp


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same(a, b):
    """equal bits (floats) / equal values (the integer num_batches_tracked)"""
    return torch.equal(bits(a), bits(b)) if a.is_floating_point() else torch.equal(a.cpu(), b.cpu())


def encoder_mask(net):
    m = torch.zeros(net.store.flat.numel(), dtype=torch.bool)
    for n in net._param_names:
        if n.startswith(ENC):
            e = net.store.entries[n]
            m[e.offset:e.offset + (e.size + 3) // 4 * 4] = True
    return m


def run(Z, steps=6, decay=None, warmup=False, freeze_after=None, seed=31, after_step=None):
    """`steps` training steps (one seeded batch per step) with a ModelEma attached when decay is given; a CPU snapshot of store.flat and
    _rmv after every step.  freeze_after = k: the encoder is frozen after step k (the later steps take the segmented Adam path)."""
    ema, optim = Z[2], Z[5]
    net, lf = build(Z, seed)
    opt = optim.FusedAdam(net, lr=1e-3, betas=(0.9, 0.99), weight_decay=1e-2)
    avg = ema.ModelEma(net, decay=decay, warmup=warmup).attach(opt) if decay is not None else None
    snaps, stats = [], []
    for it in range(steps):
        opt.zero_grad()
        lf(net(batch(seed=5 + it)), batch(seed=5 + it))["loss"].backward()
        opt.step()
        torch.cuda.synchronize()
        snaps.append(net.store.flat.cpu().clone())
        stats.append(net._rmv.cpu().clone())
        if after_step is not None:
            after_step(it, net, opt, avg)
        if freeze_after is not None and it + 1 == freeze_after:
            for n, p in net.named_parameters():
                p.requires_grad_(not n.startswith(ENC))
            net.zero_grad(set_to_none=True)
    return net, opt, avg, lf, snaps, stats


def test_attached_average_follows_the_reference_and_leaves_training_alone(Z):
    first = {}

    def after(it, net, opt, avg):
        if it == 0:
            first["flat"], first["rmv"] = avg.flat.cpu().clone(), avg.rmv.cpu().clone()
    net, opt, avg, _, snaps, stats = run(Z, decay=0.9, warmup=True, after_step=after)
    assert avg.n_averaged == 6 and not opt._seg
    # the first update is a copy
    assert torch.equal(bits(first["flat"]), bits(snaps[0])) and torch.equal(bits(first["rmv"]), bits(stats[0]))
    # the whole average against the fp64 recurrence with the warm-up schedule (decay_t = 2/11, 3/12, ... below 0.9), every element
    ref, bnd = ema_ref.trajectory(snaps, 0.9, True)
    ema_ref.assert_within(avg.flat, ref, bnd, "flat, 6 attached steps")
    ref_s, bnd_s = ema_ref.trajectory(stats, 0.9, True)
    ema_ref.assert_within(avg.rmv, ref_s, bnd_s, "BatchNorm statistics, 6 attached steps")
    assert torch.equal(avg.nbt, net._nbt) and int(net._nbt[0]) == 6
    # ... and NOT the constant-decay one: the schedule is honoured
    plain, _ = ema_ref.trajectory(snaps, 0.9, False)
    assert bool(((avg.flat.cpu().double() - plain).abs() > bnd).any())
    assert not torch.equal(bits(avg.flat), bits(snaps[-1]))
    # the run without an average on the same seeds: raw weights, moments, counter and statistics are the same bits
    net2, opt2, _, _, snaps2, stats2 = run(Z)
    for a, b in zip(snaps + stats, snaps2 + stats2):
        assert torch.equal(bits(a), bits(b)), "the weight average changed the training trajectory"
    assert torch.equal(bits(opt.m), bits(opt2.m)) and torch.equal(bits(opt.v), bits(opt2.v))
    assert opt.step_count.tolist() == opt2.step_count.tolist() == [6]
    # update() by hand while attached would count a step twice
    with pytest.raises(RuntimeError, match="attached"):
        avg.update()
    assert avg.n_averaged == 6


def test_parameter_frozen_on_the_way_keeps_converging(Z):
    net, opt, avg, lf, snaps, stats = run(Z, decay=0.5, freeze_after=3, seed=32)
    assert opt._seg and avg.n_averaged == 6, "steps 4..6 should have taken the segmented path"
    enc = encoder_mask(net)
    assert bool(enc.any()) and torch.equal(bits(snaps[2][enc]), bits(snaps[5][enc])), "the frozen encoder moved"
    assert not torch.equal(bits(snaps[2][~enc]), bits(snaps[5][~enc]))
    # the encoder's average keeps moving toward the now-constant weights: the distance halves with every update
    # (three more updates at w = 0.5; exact in the recurrence, within the trajectory bound in fp32)
    ref, bnd = ema_ref.trajectory(snaps, 0.5)
    ref3, _ = ema_ref.trajectory(snaps[:3], 0.5)
    d3 = (ref3[enc] - snaps[2][enc].double()).abs()
    d6 = (avg.flat.cpu()[enc].double() - snaps[5][enc].double()).abs()
    assert float(d3.max()) > 1e-5 and float(d6.max()) < 0.2 * float(d3.max())
    assert bool((d6 <= d3 / 8 + bnd[enc]).all())
    # the whole average still matches the reference
    ema_ref.assert_within(avg.flat, ref, bnd, "flat, encoder frozen after step 3")
    ref_s, bnd_s = ema_ref.trajectory(stats, 0.5)
    ema_ref.assert_within(avg.rmv, ref_s, bnd_s, "BatchNorm statistics, encoder frozen after step 3")
    # the explicit form, for any optimizer: detach, step, update()
    avg.detach()
    opt.zero_grad()
    lf(net(batch(seed=20)), batch(seed=20))["loss"].backward()
    opt.step()
    assert avg.n_averaged == 6
    avg.update()
    torch.cuda.synchronize()
    assert avg.n_averaged == 7
    snaps.append(net.store.flat.cpu().clone())
    ref, bnd = ema_ref.trajectory(snaps, 0.5)
    ema_ref.assert_within(avg.flat, ref, bnd, "flat, one more explicit update")


def test_applied_is_the_averaged_model_and_restores_everything(Z):
    _lib, config, ema, loss, mdl, optim = Z
    net, opt, avg, lf, snaps, stats = run(Z, steps=3, decay=0.5, seed=33)
    inp = batch(seed=40)
    net.eval()

    def forward():
        with torch.no_grad():
            out = net(inp)
        torch.cuda.synchronize()
        return {k: out[k].detach().clone() for k in ("att_bbx_out",)}
    raw_out = forward()
    esd = {k: (v.detach().clone() if isinstance(v, torch.Tensor) else v) for k, v in avg.state_dict().items()}
    meta = esd.pop(ema.META_KEY)
    assert meta == dict(n_averaged=3, decay=0.5, warmup=False)
    rsd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    keep = dict(flat=net.store.flat.clone(), rmv=net._rmv.clone(), nbt=net._nbt.clone(), m=opt.m.clone(), v=opt.v.clone(),
                cnt=opt.step_count.clone(), eflat=avg.flat.clone(), ermv=avg.rmv.clone(), enbt=avg.nbt.clone())
    assert any(not same(esd[k], rsd[k]) for k in esd)
    ptrs = (net.store.flat.data_ptr(), net._rmv.data_ptr(), avg.flat.data_ptr())
    with avg.applied() as inside:
        assert inside is avg
        nsd = net.state_dict()
        assert list(nsd) == list(esd)
        for k in esd:
            assert same(nsd[k], esd[k]), k
        in_out = forward()
        with pytest.raises(RuntimeError, match="applied"):
            opt.step()
        with pytest.raises(RuntimeError):
            avg.update()
        avg.detach()
        with pytest.raises(RuntimeError, match="applied"):
            avg.update()
        with pytest.raises(RuntimeError, match="applied"):
            with avg.applied():
                pass
        with pytest.raises(RuntimeError, match="applied"):
            avg.reset()
        avg.attach(opt)
    torch.cuda.synchronize()
    assert avg.n_averaged == 3 and net.__dict__.get("_ema_applied") is None
    assert ptrs == (net.store.flat.data_ptr(), net._rmv.data_ptr(), avg.flat.data_ptr())          # contents moved, buffers stayed
    now = dict(flat=net.store.flat, rmv=net._rmv, nbt=net._nbt, m=opt.m, v=opt.v, cnt=opt.step_count, eflat=avg.flat, ermv=avg.rmv,
               enbt=avg.nbt)
    for k, t in keep.items():
        assert same(now[k], t), k
    assert not torch.equal(in_out["att_bbx_out"], raw_out["att_bbx_out"])
    assert torch.equal(bits(forward()["att_bbx_out"]), bits(raw_out["att_bbx_out"]))
    # an exception inside still restores
    with pytest.raises(KeyError):
        with avg.applied():
            raise KeyError("x")
    torch.cuda.synchronize()
    assert torch.equal(bits(net.store.flat), bits(keep["flat"])) and torch.equal(bits(avg.flat), bits(keep["eflat"]))
    # the same network with the average loaded as its weights computes the same bits as inside applied()
    net.load_state_dict(esd)
    assert torch.equal(bits(forward()["att_bbx_out"]), bits(in_out["att_bbx_out"]))
    net.load_state_dict(rsd)
    # a store that moved since the average was taken is refused, reset() takes the new one
    old = net.store.flat          # (kept alive: the allocator cannot hand the same block out again)
    avg.detach()
    net.to("cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        avg.update()
    net.to("cuda")
    with pytest.raises(RuntimeError, match="moved or reallocated"):
        avg.update()
    assert old.data_ptr() != net.store.flat.data_ptr()
    avg.reset()
    avg.update()
    torch.cuda.synchronize()
    assert avg.n_averaged == 1 and torch.equal(bits(avg.flat), bits(net.store.flat))


def _launches(L, fn):
    L.lib.zsg_prof_enable(1)
    try:
        L.lib.zsg_prof_collect((L.ProfEntry * 256)(), 256)          # (drop earlier records)
        fn()
        torch.cuda.synchronize()
        ents = (L.ProfEntry * 256)()
        n = L.lib.zsg_prof_collect(ents, 256)
    finally:
        L.lib.zsg_prof_enable(0)
    return {ents[i].name.decode(): ents[i].launches for i in range(n)}


def _learner(Z, tmp_path, uid, **kw):
    config = Z[1]
    from zsgnet_pytorch_amd.main_dist import learner_init
    cfg = config.get_cfg(resnet_arch="resnet18", bs=2, bsv=2, resize_img=[96, 96], steps_per_epoch=5, tmp_path=str(tmp_path), synthetic=True,
                         **kw)
    cfg.freeze()
    return learner_init(uid, cfg)


def test_learner_trains_validates_checkpoints_and_resumes_with_the_average(Z, tmp_path):
    L, ema = Z[0], Z[2]
    learn = _learner(Z, tmp_path, "ema", ema_decay=0.9)
    assert learn.ema is None
    learn.fit(epochs=2, lr=1e-3)
    avg = learn.ema
    assert avg is not None and avg.n_averaged == 10 and learn.optimizer._ema is avg and (avg.decay, avg.warmup) == (0.9, False)
    assert not torch.equal(bits(avg.flat), bits(learn.mdl.store.flat))
    # one step's optimizer launches: the fused step and the statistics' update, nothing else of the family
    learn.data.train_dl.steps = 1
    got = _launches(L, learn.train_epoch)
    assert got.get("adam_step_ema") == 1 and got.get("ema_update") == 1, got
    assert not {"adam_step", "adam_step_segments", "swap_f32"} & set(got), got
    assert avg.n_averaged == 11
    # validate reports the averaged model's numbers: those of a by-hand validation under applied(), not the raw weights'
    torch.manual_seed(0)
    va = learn.validate()
    learn.ema = None
    try:
        torch.manual_seed(0)
        with avg.applied():
            by_hand = learn.validate()
        torch.manual_seed(0)
        raw = learn.validate()
    finally:
        learn.ema = avg
    print("validate:", va, "raw weights:", raw)
    assert va == by_hand
    assert va["loss"] != raw["loss"]
    # the checkpoint: raw weights under model_state_dict, the average beside them
    learn.save_model_dict()
    ck = torch.load(learn.model_file, map_location="cpu")
    assert "ema_state_dict" in ck and ck["ema_state_dict"][ema.META_KEY] == dict(n_averaged=11, decay=0.9, warmup=False)
    nsd, esd = learn.mdl.state_dict(), avg.state_dict()
    assert list(ck["ema_state_dict"]) == list(nsd) + [ema.META_KEY]
    for k in nsd:
        assert torch.equal(ck["model_state_dict"][k], nsd[k].cpu()), k
        assert torch.equal(ck["ema_state_dict"][k], esd[k].cpu()), k
    # a fresh Learner resumes with an equal average (before any optimizer exists: --only_val evaluates it), and keeps updating it
    again = _learner(Z, tmp_path, "ema", ema_decay=0.9)
    assert again.num_it == learn.num_it and again.ema is not None and again.optimizer is None
    assert again.ema.n_averaged == 11
    assert torch.equal(bits(again.ema.flat), bits(avg.flat)) and torch.equal(bits(again.ema.rmv), bits(avg.rmv))
    assert torch.equal(again.ema.nbt, avg.nbt)
    assert torch.equal(bits(again.mdl.store.flat), bits(learn.mdl.store.flat))
    torch.manual_seed(0)
    assert again.validate() == va
    again.prepare_optimizer(1e-3)
    assert again.optimizer._ema is again.ema and again.ema.n_averaged == 11
    # a checkpoint without an average: it starts from the loaded weights
    del ck["ema_state_dict"]
    torch.save(ck, learn.model_file)
    third = _learner(Z, tmp_path, "ema", ema_decay=0.9, ema_eval=False)
    assert third.ema.n_averaged == 0 and torch.equal(bits(third.ema.flat), bits(third.mdl.store.flat))
    torch.manual_seed(0)
    assert third.validate() == raw          # ema_eval off: the raw weights are validated


def test_learner_without_ema_is_unchanged(Z, tmp_path):
    L = Z[0]
    learn = _learner(Z, tmp_path, "plain")
    learn.fit(epochs=1, lr=1e-3)
    assert learn.ema is None and learn.optimizer._ema is None
    learn.data.train_dl.steps = 1
    got = _launches(L, learn.train_epoch)
    assert got.get("adam_step") == 1, got
    assert not {"adam_step_ema", "ema_update", "swap_f32"} & set(got), got
    got = _launches(L, learn.validate)
    assert not {"adam_step_ema", "ema_update", "swap_f32"} & set(got), got
    learn.save_model_dict()
    ck = torch.load(learn.model_file, map_location="cpu")
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "num_it", "num_epoch", "cfgtxt", "best_met"}

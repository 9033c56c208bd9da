"""mobgs_amd.checkpoint on the device: the snapshot / restore kernels bit for bit (include/mobgs_hip.h K29), and a training
run that is stopped, saved, dropped, loaded and continued against the same run left alone.  Every comparison is exact
(torch.equal, equal Python floats): a copy and a replayed computation have no tolerance."""
import gc
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

from mobgs_amd import checkpoint as C  # noqa: E402

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000
GUARD_WORDS = 64


# ---- 1. the two kernels ---------------------------------------------------------------------------------------------------
def _table(dev, n, cap, seed):
    """Fields of row sizes 1 (the uint8 table), 4, 12, 36, 144, 8 (integer counts), 6 (fp16) and a 12-byte field whose view
    starts one row into its buffer (4-byte aligned only); every buffer has cap rows + one guard row."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(cap + 1, *s, generator=g)  # noqa: E731
    specs = [("table", torch.randint(0, 2, (cap + 1,), generator=g).to(torch.uint8), False),
             ("f4", rnd(1), True), ("xyz12", rnd(3), False), ("m36", rnd(9), True), ("c144", rnd(12, 3), False),
             ("knots8", torch.randint(2, 13, (cap + 1, 1), generator=g), False), ("half6", rnd(3).half(), True)]
    fields = [(name, t.to(dev), zn) for name, t, zn in specs]
    shifted = rnd(3)
    extra = torch.cat([torch.zeros(1, 3), shifted]).to(dev)   # rows 1 .. cap + 1 are the field: starts 12 bytes in
    fields.append(("shift12", extra[1:], True))
    assert extra[1:].data_ptr() % 16 == 12
    return fields


def _row_bytes(t):
    return (t[0].numel() if t.dim() > 1 else 1) * t.element_size()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_snapshot_and_restore_move_every_field_bit_for_bit(hip_device, n):
    dev, cap = hip_device, n + 37
    src = _table(dev, n, cap, seed=n)
    rb = [_row_bytes(t) for _, t, _ in src]
    assert sorted(rb) == [1, 4, 6, 8, 12, 12, 36, 144]
    offsets, total = C.pack_layout(rb, n)
    zero_new = [zn for _, _, zn in src]
    _, recs = C._upload(C.field_records([t.data_ptr() for _, t, _ in src], rb, offsets, zero_new))
    # a block from NaN-poisoned memory with guard words behind it
    words = torch.full((total // 4 + GUARD_WORDS,), float("nan"), device=dev)
    assert int(words.view(torch.int32)[0]) == NAN_BITS
    block = words.view(torch.uint8)
    s = torch.zeros(1, dtype=torch.int64, device=dev)
    C.rows_snapshot(recs, len(src), n, max(rb), block, s)
    torch.cuda.synchronize()
    inside, guard = words[:total // 4], words[total // 4:]
    assert not bool(torch.isnan(inside).any()), "an unwritten (poisoned) word inside [0, total_bytes)"
    assert bool((guard.view(torch.int32) == NAN_BITS).all()), "the guard words behind total_bytes were written"
    host = block[:total].cpu().numpy()
    want = int(host.view("<u4").sum(dtype=np.uint64))
    assert (int(s.item()) & (2 ** 64 - 1)) == want == C.word_sum(host)
    for (name, t, _), off, b in zip(src, offsets, rb):       # the packed layout itself
        assert bytes(host[off:off + n * b]) == t[:n].contiguous().cpu().numpy().tobytes(), name
        assert not host[off + n * b:off + C.round16(n * b)].any(), (name, "slot padding")

    # restore into sentinel-filled buffers of the same geometry (the shifted one included)
    dst = _table(dev, n, cap, seed=1000 + n)
    before = [t.clone() for _, t, _ in dst]
    _, drecs = C._upload(C.field_records([t.data_ptr() for _, t, _ in dst], rb, offsets, zero_new))
    C.rows_restore(drecs, len(dst), n, cap, max(rb), block)
    torch.cuda.synchronize()
    for (name, t, zn), (_, s_t, _), old in zip(dst, src, before):
        assert torch.equal(t[:n], s_t[:n]), (name, "rows [0, n)")
        if zn:
            assert not bool(t[n:cap].any()), (name, "rows [n, capacity) of a zero_new field must be zero")
        else:
            assert torch.equal(t[n:cap], old[n:cap]), (name, "rows [n, capacity) of the other fields are left alone")
        assert torch.equal(t[cap:], old[cap:]), (name, "the guard row behind the capacity was written")


def test_entry_points_refuse_bad_arguments(hip_device):
    dev = hip_device
    t = torch.zeros(16, 3, device=dev)
    _, recs = C._upload(C.field_records([t.data_ptr()], [12], [0], [False]))
    block = torch.zeros(4096, dtype=torch.uint8, device=dev)
    s = torch.zeros(1, dtype=torch.int64, device=dev)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        C.rows_snapshot(recs, 1, 16, 12, block[4:], s)
    with pytest.raises(RuntimeError, match="bad arguments"):
        C.rows_snapshot(recs, 1, -1, 12, block, s)
    with pytest.raises(RuntimeError, match="capacity"):
        C.rows_restore(recs, 1, 16, 8, 12, block)
    torch.cuda.synchronize()
    assert int(s.item()) == 0 and not bool(block.any())


# ---- 2. resume is bit-identical -----------------------------------------------------------------------------------------
# 256 x 192, 3000 + 1500 splats growing by a tenth per densification (at most 4000 + 2000), lambda_flow_loss = 0 (the shipped
# seesaw setting: the flow loss's float atomics are not ordered from run to run), 12 iterations with a densification and an
# opacity reset on either side of the save point, and one exposure-time estimate before it.
SETTINGS = dict(iters=12, ns=3000, nd=1500, width=256, height=192, seed=3, lambda_flow=0.0, densify_at=(4, 9),
                reset_opacity_at=(5, 10), estimate_exposure_at=(3,))
SAVE_AT = 6


def _optimizer_state(opt):
    out = {}
    for gi, g in enumerate(opt.param_groups):
        out[f"{g['name']}.lr"] = torch.tensor(g["lr"], dtype=torch.float64)
        for pj, p in enumerate(g["params"]):
            for k, v in (opt.state.get(p) or {}).items():
                out[f"{g['name']}.{gi}.{pj}.{k}"] = torch.as_tensor(v).detach().cpu().clone()
    return out


def _everything(t):
    """What a continued run must reproduce: both tables, decoder and BLCE parameters (exposure_time_expo among them), all
    moments and step counts, every group's rate."""
    out = {}
    for name, pc in (("stat", t.stat), ("dyn", t.dyn)):
        out.update({f"{name}.{k}": v.detach().cpu().clone() for k, v in pc.table_state().items()})
        out.update({f"{name}.decoder.{k}": v.detach().cpu().clone() for k, v in pc.rgbdecoder.state_dict().items()})
        out.update({f"{name}.opt.{k}": v for k, v in _optimizer_state(pc.optimizer).items()})
    out.update({f"blce.{k}": v.detach().cpu().clone() for k, v in t.blce.state_dict().items()})
    out.update({f"blce.opt.{k}": v for k, v in _optimizer_state(t.blce.optimizer).items()})
    out["blce.lr_factor"] = torch.tensor(t.blce.lr_factor, dtype=torch.float64)
    return out


def _assert_same(a, b, what):
    assert a.keys() == b.keys(), (what, sorted(set(a) ^ set(b)))
    bad = [k for k in a if a[k].shape != b[k].shape or not torch.equal(a[k], b[k])]
    assert not bad, (what, bad[:12], len(bad))


_straight = {}


def _straight_run(dev, graph):
    """The uninterrupted run, computed once per variant and left unchanged."""
    if graph not in _straight:
        import resume_deblur_synth as R
        history, t, _, fit = R.run(dev=str(dev), graph=graph, **SETTINGS)
        assert fit, "an arena was outgrown during a replay: the straight run is not a valid yardstick"
        _straight[graph] = (history, _everything(t), (t.stat._n, t.dyn._n))
        del t
        gc.collect()
    return _straight[graph]


def test_two_straight_runs_agree(hip_device):
    """The precondition that makes the comparison below meaningful: the loop at these settings is deterministic."""
    import resume_deblur_synth as R
    history, state, rows = _straight_run(hip_device, False)
    again, t, _, _ = R.run(dev=str(hip_device), **SETTINGS)
    assert rows[0] > SETTINGS["ns"] and rows[1] > SETTINGS["nd"], ("the densifications must have added rows", rows)
    assert rows[0] <= 4000 and rows[1] <= 2000, rows
    assert history == again, (history, again)
    _assert_same(state, _everything(t), "two straight runs")


@pytest.mark.parametrize("graph", [False, True], ids=["eager_fused_adam", "graphed_device_adam"])
def test_resumed_run_is_bit_identical(hip_device, tmp_path, graph):
    """Run to 6, save, drop every object, load into fresh ones, run to 12: tables, decoder and BLCE parameters, moments, step
    counts, rates, exposure_time_expo and the losses of iterations 7 to 12 equal the uninterrupted run's.  graph=True: the
    iteration with its DeviceAdam step replayed from a graph, the device counters rebuilt from the restored step counts
    and the graph recorded again after the load."""
    import resume_deblur_synth as R
    dev = str(hip_device)
    history, state, rows = _straight_run(hip_device, graph)
    path = str(tmp_path / "run.mobgs")
    first, t, handles, fit = R.run(dev=dev, graph=graph, path=path, save_at=(SAVE_AT,), stop_at=SAVE_AT, **SETTINGS)
    assert fit and first == history[:SAVE_AT] and handles[0].result() == path
    del t, handles
    gc.collect()
    torch.manual_seed(987654321)          # (whatever the generators hold now must not matter)
    torch.cuda.manual_seed(123)
    rest, t, _, fit = R.run(dev=dev, graph=graph, resume=path, **SETTINGS)
    assert fit
    assert rest == history[SAVE_AT:], (rest, history[SAVE_AT:])
    assert (t.stat._n, t.dyn._n) == rows
    _assert_same(state, _everything(t), "resumed against straight")


# ---- 3. a save does not see later steps ---------------------------------------------------------------------------------
SMALL = dict(iters=8, ns=1500, nd=800, width=160, height=112, seed=5, lambda_flow=0.0)


def test_asynchronous_save_holds_the_state_of_its_iteration(hip_device, tmp_path):
    """save(blocking=False) at iteration 3, three more iterations before the handle is waited for: the file equals the one a
    twin run wrote with a blocking save at 3 and stopped."""
    import resume_deblur_synth as R
    a, b = str(tmp_path / "async.mobgs"), str(tmp_path / "blocking.mobgs")
    _, ta, handles, _ = R.run(dev=str(hip_device), path=a, save_at=(3,), stop_at=6, **SMALL)   # (waits at the end)
    assert handles[0].done()
    _, tb, _, _ = R.run(dev=str(hip_device), path=b, save_at=(3,), stop_at=3, blocking=True, **SMALL)
    ha, ba = C.read_checkpoint(a)
    hb, bb = C.read_checkpoint(b)
    assert ha == hb
    for k in bb:
        assert np.array_equal(ba[k], bb[k]), k
    # ... and it is not the state three iterations later
    assert not torch.equal(ta.stat._xyz.detach(), tb.stat._xyz.detach())
    loaded = C.load_training_state(a, device=hip_device, training_args=tb.opt, set_generators=False)
    for name in ("stat", "dyn"):
        want, got = getattr(tb, name).table_state(), getattr(loaded, name).table_state()
        assert want.keys() == got.keys()
        assert all(torch.equal(want[k], got[k]) for k in want), name


# ---- 4. interchange -----------------------------------------------------------------------------------------------------
def test_export_reference_layout_round_trips_through_from_ply(hip_device, tmp_path):
    import resume_deblur_synth as R
    from mobgs_amd.densify import GROUPS, TrainableGaussians
    path = str(tmp_path / "run.mobgs")
    _, t, _, _ = R.run(dev=str(hip_device), path=path, save_at=(2,), stop_at=2, blocking=True, **SMALL)
    out = C.export_reference_layout(tmp_path / "point_cloud" / "iteration_2", stat=t.stat, dyn=t.dyn, blce=t.blce)
    assert sorted(os.path.basename(p) for p in out) == ["blce.pth", "point_cloud.ply", "point_cloud.pt",
                                                        "point_cloud_static.ply"]
    loaded = C.load_training_state(path, device=hip_device, training_args=t.opt, set_generators=False)
    for ply, pc in ((out[0], loaded.dyn), (out[1], loaded.stat)):
        back = TrainableGaussians.from_ply(ply, device=hip_device)
        for _, attr in GROUPS:
            assert torch.equal(getattr(back, attr).detach(), getattr(pc, attr).detach()), (ply, attr)
        for k, v in pc.rgbdecoder.state_dict().items():
            assert torch.equal(back.rgbdecoder.state_dict()[k], v), (ply, k)
    blce = torch.load(os.path.join(os.path.dirname(out[0]), "blce.pth"), map_location=hip_device)
    for k, v in loaded.blce.model.state_dict().items():
        assert torch.equal(blce[k], v), k
    # the thin wrappers: state_dict() of one set into a fresh set of another row count
    sd = t.dyn.state_dict()
    fresh = TrainableGaussians.from_ply(out[1], device=hip_device)      # (the static set's rows: another n)
    fresh.load_state_dict(sd)
    want = t.dyn.table_state()
    got = fresh.table_state()
    assert all(torch.equal(want[k], got[k]) for k in got) and set(got) <= set(want)
    for k in C.STATS:
        assert not bool(fresh._fields[k].buf[fresh._fields[k].cur][fresh._n:].any()), k

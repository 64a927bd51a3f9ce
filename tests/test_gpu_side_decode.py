"""GPU: the decoder on its own stream, launched behind the next batch's reader (FusedPillarNeXt.decode_on_side_stream, the default; fused._DeferredDecode)
in a pipelined serving loop returns the same detections, bit for bit, as the single-stream loop -- also when a result is asked for before the next
batch is enqueued (the deferred launch is flushed) and when a pending result is dropped."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def test_side_stream_decode_equals_single_stream():
    from pillarnext_amd import synth
    from pillarnext_amd.models import FusedPillarNeXt, build_pillarnext_b

    cfg = synth.CONFIGS["C2"]
    torch.manual_seed(0)
    det = build_pillarnext_b(cfg["pc_range"], cfg["voxel_size"]).cuda().eval()
    model = FusedPillarNeXt(det).cuda().eval()
    exs = []
    for k in range(3):
        pts = torch.from_numpy(synth.make_batch("C2", 2, "sweep", frame0=2 * k, n=120_000)).cuda()
        exs.append({"points": pts, "token": [f"b{k}f{i}" for i in range(2)], "batch_size": 2})

    def loop():
        outs, pending = [], None
        for i in range(6):
            nxt = model.forward_async(exs[i % 3])
            if pending is not None:
                outs.append(model.detections(pending.result()))
            pending = nxt
        outs.append(model.detections(pending.result()))
        return outs

    model.decode_on_side_stream = False
    ref = loop()
    model.decode_on_side_stream = True
    got = loop()
    torch.cuda.synchronize()
    assert len(ref) == len(got) == 6
    for a, b in zip(ref, got):
        assert set(a) == set(b)
        for tok in a:
            assert len(a[tok]["scores"]) > 0
            for k in ("box3d_lidar", "scores", "label_preds"):
                assert torch.equal(a[tok][k], b[tok][k]), (tok, k)


def test_deferred_decode_is_flushed_by_result_and_survives_a_dropped_pending():
    from pillarnext_amd import synth
    from pillarnext_amd.fused import _DeferredDecode
    from pillarnext_amd.models import FusedPillarNeXt, build_pillarnext_b

    cfg = synth.CONFIGS["C2"]
    torch.manual_seed(0)
    model = FusedPillarNeXt(build_pillarnext_b(cfg["pc_range"], cfg["voxel_size"]).cuda().eval()).cuda().eval()
    assert model.decode_on_side_stream
    pts = torch.from_numpy(synth.make_batch("C2", 1, "sweep", n=100_000)).cuda()
    ex = {"points": pts, "token": ["a"], "batch_size": 1}
    p1 = model.forward_async(ex)
    assert isinstance(p1, _DeferredDecode) and not p1.launched
    r1 = model.detections(p1.result())                     # nobody enqueued a next batch: result() launches the decoder itself
    assert p1.launched and int(p1.flag_h[0]) in (0, 1)
    model.forward_async(ex)                                 # dropped without result(): held by weak reference only, so it is never launched and its maps are freed
    assert model.__dict__["_deferred"]() is None
    r3 = model(ex)
    model.decode_on_side_stream = False
    r4 = model(ex)
    for r in (r3, r4):
        assert torch.equal(r["a"]["scores"], r1["a"]["scores"]) and torch.equal(r["a"]["box3d_lidar"], r1["a"]["box3d_lidar"])
    # copy.deepcopy / torch.save of the module: the side stream and the pending decoder are launch state, not model state
    import copy
    import io

    kept = model.forward_async(ex)                          # a live pending handle and a live side stream while the module is copied
    twin = copy.deepcopy(model)
    torch.save(model, io.BytesIO())
    assert "_decode_stream" not in twin.__dict__ and "_deferred" not in twin.__dict__
    model.decode_on_side_stream = twin.decode_on_side_stream = True
    r5, r6 = model.detections(kept.result()), twin(ex)
    assert torch.equal(r5["a"]["scores"], r1["a"]["scores"]) and torch.equal(r6["a"]["scores"], r1["a"]["scores"])

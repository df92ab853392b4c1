"""CPU: averaged weights (TrainStep(ema_decay > 0)) -- checkpoint round trips, average_checkpoints against NumPy fp64, and what the
constructor and retune refuse.  The flat buffers work on any device; nothing here calls the library."""
import warnings

import numpy as np
import pytest
import torch

from test_host_logic import models

DIMS = (50, 60, 96, 16, 16, 24, 20, 0.99)


def _model(seed):
    V11, _ = models()
    torch.manual_seed(seed)
    return V11(*DIMS, tied_emb=True)


def _driver(seed, **kw):
    from vagnmt_hip.trainer import TrainStep
    m = _model(seed)
    return m, TrainStep(m, None, None, use_graph=False, **kw)


def _slices(ts, buf):
    fp = ts.fp
    return {n: buf[fp.offsets[n]:fp.offsets[n] + p.numel()] for n, p in fp.named}


def test_ema_decay_zero_allocates_no_fifth_buffer():
    _, ts = _driver(0)
    assert ts.ema_decay == 0.0 and ts.fp.ema is None and ts.fp.ema_alloc is None and len(ts.fp._alloc) == 4
    with pytest.raises(RuntimeError):
        ts.ema_state_dict()
    with pytest.raises(RuntimeError):
        with ts.averaged_weights():
            pass
    _, te = _driver(0, ema_decay=0.99)
    assert len(te.fp._alloc) == 5 and te.fp.ema.shape == te.fp.flat.shape and te.fp.ema.dtype == torch.float32
    assert te.fp.ema.data_ptr() != te.fp.flat.data_ptr() and te.fp.ema.data_ptr() % 16 == 0
    assert torch.equal(te.fp.ema, te.fp.flat)                  # the average starts at the parameters


def test_checkpoint_roundtrip_of_the_averaged_weights(tmp_path):
    from vagnmt_hip.checkpoint import load_checkpoint, save_checkpoint
    m, ts = _driver(0, ema_decay=0.99)
    ts.fp.ema.copy_(torch.randn_like(ts.fp.ema))
    ts.fp.m.copy_(torch.randn_like(ts.fp.m))
    ts.step_count.fill_(5)
    path = str(tmp_path / "ck.pt")
    ck = save_checkpoint(path, m, ts)
    assert ck["format"] == "vag-nmt-checkpoint-v1" and ck["ema"]["decay"] == 0.99 and ck["ema"]["warmup"] is True
    assert sorted(ck["ema"]["params"]) == sorted(n for n, _ in ts.fp.named)
    m2, ts2 = _driver(1, ema_decay=0.99)
    before = ts2.fp.ema.data_ptr()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        load_checkpoint(path, m2, ts2)
    assert ts2.fp.ema.data_ptr() == before                     # in place: captured graphs hold this address
    a, b = _slices(ts, ts.fp.ema), _slices(ts2, ts2.fp.ema)
    for n in a:
        assert torch.equal(a[n], b[n]), n
    assert torch.equal(ts2.fp.flat, ts.fp.flat) and int(ts2.step_count) == 5
    # the raw parameters of the source were left alone, and they differ from the average
    assert not torch.equal(ts.fp.ema, ts.fp.flat)

    # ema_state_dict: reference names, tied weights as in model.state_dict(), CPU tensors of the average
    esd = ts.ema_state_dict()
    assert list(esd) == list(m.state_dict())
    for n, p in ts.fp.named:
        assert torch.equal(esd[n], a[n].view_as(p)), n
    assert "decoder.out.weight" in esd and torch.equal(esd["decoder.out.weight"], esd["decoder.embedding.weight"])

    # use_ema=True into a bare model equals ema_state_dict()
    m3 = _model(2)
    load_checkpoint(path, m3, use_ema=True)
    sd3 = m3.state_dict()
    for k in esd:
        assert torch.equal(sd3[k], esd[k]), k
    # ... and without it the raw parameters
    m4 = _model(3)
    load_checkpoint(path, m4)
    for k, v in m.state_dict().items():
        assert torch.equal(m4.state_dict()[k], v), k

    with pytest.raises(ValueError):
        load_checkpoint(path, m2, ts2, use_ema=True)


def test_checkpoint_without_an_average(tmp_path):
    from vagnmt_hip.checkpoint import load_checkpoint, save_checkpoint
    m, ts = _driver(0)
    ts.fp.m.copy_(torch.randn_like(ts.fp.m))
    path = str(tmp_path / "plain.pt")
    ck = save_checkpoint(path, m, ts)
    assert "ema" not in ck
    m2, ts2 = _driver(1, ema_decay=0.9)
    ts2.fp.ema.copy_(torch.randn_like(ts2.fp.ema))
    before = ts2.fp.ema.data_ptr()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        load_checkpoint(path, m2, ts2)
    assert len([w for w in rec if "averaged weights" in str(w.message)]) == 1
    assert ts2.fp.ema.data_ptr() == before
    a, b = _slices(ts2, ts2.fp.ema), _slices(ts2, ts2.fp.flat)
    for n in a:
        assert torch.equal(a[n], b[n]), n
    assert torch.equal(ts2.fp.flat, ts.fp.flat)
    with pytest.raises(KeyError):
        load_checkpoint(path, _model(2), use_ema=True)
    # a bare state_dict and a pickled module hold no average either
    torch.save(dict(m.state_dict()), str(tmp_path / "sd.pt"))
    with pytest.raises(KeyError):
        load_checkpoint(str(tmp_path / "sd.pt"), _model(2), use_ema=True)
    # an averaging checkpoint loads into a driver that keeps no average (older readers ignore the key)
    me, te = _driver(4, ema_decay=0.9)
    save_checkpoint(str(tmp_path / "e.pt"), me, te)
    m5, ts5 = _driver(5)
    load_checkpoint(str(tmp_path / "e.pt"), m5, ts5)
    assert ts5.fp.ema is None and torch.equal(ts5.fp.flat, te.fp.flat)


def test_nothing_trains_or_checkpoints_inside_the_averaged_block(tmp_path):
    from vagnmt_hip._lib import VagError
    from vagnmt_hip.checkpoint import load_checkpoint, save_checkpoint
    m, ts = _driver(0, ema_decay=0.9)
    path = str(tmp_path / "ck.pt")
    save_checkpoint(path, m, ts)
    flat = ts.fp.flat.clone()
    with pytest.raises(VagError):                 # the exchange is the library's: CPU buffers are refused, nothing has moved
        with ts.averaged_weights():
            pass
    assert ts._averaged is False and torch.equal(ts.fp.flat, flat) and torch.equal(ts.fp.ema, flat)
    ts._averaged = True                           # (the state inside the block)
    for fn in (lambda: ts.step(None, [1], None), lambda: ts.mrt_step(None, [1], None), ts.reset_ema,
               lambda: save_checkpoint(path, m, ts), lambda: load_checkpoint(path, m, ts)):
        with pytest.raises(RuntimeError, match="averaged_weights"):
            fn()
    with pytest.raises(RuntimeError, match="nested"):
        with ts.averaged_weights():
            pass


def test_reset_ema_is_in_place():
    _, ts = _driver(0, ema_decay=0.5)
    ts.fp.ema.copy_(torch.randn_like(ts.fp.ema))
    before = ts.fp.ema.data_ptr()
    ts.reset_ema()
    assert ts.fp.ema.data_ptr() == before and torch.equal(ts.fp.ema, ts.fp.flat)


def test_average_checkpoints_against_numpy_fp64(tmp_path):
    """Three checkpoints, one of each accepted form, weights [1, 2, 1]."""
    from vagnmt_hip.checkpoint import average_checkpoints, save_checkpoint
    ms = [_model(s) for s in (0, 1, 2)]
    paths = [str(tmp_path / n) for n in ("a.pt", "b.pt", "c.pt")]
    save_checkpoint(paths[0], ms[0])                                        # this project's format
    torch.save({k: v.clone() for k, v in ms[1].state_dict().items()}, paths[1])      # a bare state_dict
    torch.save(ms[2], paths[2])                                             # a pickled module
    w = [1.0, 2.0, 1.0]
    got = average_checkpoints(paths, weights=w)
    sds = [{k: v.numpy().astype(np.float64) for k, v in m.state_dict().items()} for m in ms]
    assert list(got) == list(ms[0].state_dict())
    for k in sds[0]:
        want = (sds[0][k] * (w[0] / 4.0) + sds[1][k] * (w[1] / 4.0)) + sds[2][k] * (w[2] / 4.0)      # fp64, list order
        assert got[k].dtype == torch.float32 and got[k].shape == ms[0].state_dict()[k].shape
        assert np.array_equal(got[k].numpy(), want.astype(np.float32)), k
    # no weights: the plain mean
    plain = average_checkpoints(paths[:2])
    k = "decoder.attn.v"
    assert np.array_equal(plain[k].numpy(), (sds[0][k] * 0.5 + sds[1][k] * 0.5).astype(np.float32))
    # the result loads into a model
    ms[0].load_state_dict(got)

    V11, _ = models()
    torch.manual_seed(3)
    other = V11(50, 60, 96, 16, 16, 28, 20, 0.99, tied_emb=True)           # another hidden size: shapes differ
    torch.save(dict(other.state_dict()), str(tmp_path / "shape.pt"))
    with pytest.raises(ValueError):
        average_checkpoints([paths[0], str(tmp_path / "shape.pt")])
    sd = dict(ms[1].state_dict())
    sd["not.a.parameter"] = sd.pop("decoder.attn.v")
    torch.save(sd, str(tmp_path / "name.pt"))
    with pytest.raises(ValueError):
        average_checkpoints([paths[0], str(tmp_path / "name.pt")])
    for bad in ([1.0, -1.0, 0.0], [0.0, 0.0, 0.0], [1.0, float("nan"), 1.0], [1.0, float("inf"), 1.0], [1.0, 1.0]):
        with pytest.raises(ValueError):
            average_checkpoints(paths, weights=bad)
    with pytest.raises(KeyError):
        average_checkpoints(paths, use_ema=True)                            # none of them stores an average


def test_average_checkpoints_of_stored_averages(tmp_path):
    from vagnmt_hip.checkpoint import average_checkpoints, save_checkpoint
    paths, want = [], None
    for s in (0, 1):
        m, ts = _driver(s, ema_decay=0.9)
        ts.fp.ema.copy_(torch.randn_like(ts.fp.ema))
        paths.append(str(tmp_path / ("e%d.pt" % s)))
        save_checkpoint(paths[-1], m, ts)
        e = {k: v.numpy().astype(np.float64) * 0.5 for k, v in ts.ema_state_dict().items()}
        want = e if want is None else {k: want[k] + e[k] for k in e}
    got = average_checkpoints(paths, use_ema=True)
    for k in want:
        assert np.array_equal(got[k].numpy(), want[k].astype(np.float32)), k
    assert torch.equal(got["decoder.out.weight"], got["decoder.embedding.weight"])      # tied names carry the average too


@pytest.mark.parametrize("decay", [1.0, -0.1, float("nan"), 1.5, float("inf")])
def test_constructor_and_retune_refuse_a_decay_outside_the_open_interval(decay):
    from vagnmt_hip.trainer import TrainStep
    m = _model(0)
    flat_before = [p.data_ptr() for p in m.parameters()]
    with pytest.raises(ValueError):
        TrainStep(m, None, None, use_graph=False, ema_decay=decay)
    assert [p.data_ptr() for p in m.parameters()] == flat_before           # refused before the parameters were re-homed
    _, ts = _driver(0, ema_decay=0.9)
    with pytest.raises(ValueError):
        ts.retune(ema_decay=decay)
    assert ts.ema_decay == 0.9


def test_zero1_and_foreign_optimizers_are_refused_with_a_decay():
    from vagnmt_hip.trainer import TrainStep

    class OwnOptimizer:
        phased = False

        def optimizer(self):
            raise AssertionError("never called")

    with pytest.raises(ValueError, match="zero1"):
        TrainStep(_model(0), None, None, use_graph=False, zero1=True, ema_decay=0.9)
    with pytest.raises(ValueError, match="optimizer"):
        TrainStep(_model(0), None, None, use_graph=False, backend=OwnOptimizer(), ema_decay=0.9)
    TrainStep(_model(0), None, None, use_graph=False, backend=OwnOptimizer())          # (without a decay both are fine)
    TrainStep(_model(0), None, None, use_graph=False, zero1=True)


def test_retune_changes_the_decay_by_value_and_never_switches_averaging():
    _, ts = _driver(0, ema_decay=0.9)
    ts._graphs["x"] = {}
    ts._opt_graphs["x"] = object()
    assert ts.retune(ema_decay=0.9, ema_warmup=True) is False and "x" in ts._graphs
    assert ts.retune(ema_decay=0.99) is True and ts.ema_decay == 0.99 and not ts._graphs and not ts._opt_graphs
    ts._graphs["x"] = {}
    assert ts.retune(ema_warmup=False) is True and ts.ema_warmup is False and not ts._graphs
    with pytest.raises(ValueError):
        ts.retune(ema_decay=0.0)
    _, t0 = _driver(1)
    with pytest.raises(ValueError):
        t0.retune(ema_decay=0.5)
    assert t0.retune(ema_decay=0.0) is False and t0.fp.ema is None


def test_train_shim_averaged_weights_is_a_no_op_without_a_driver():
    import train
    m = _model(0)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    with train.averaged_weights(m):
        for k, v in m.state_dict().items():
            assert torch.equal(v, sd[k])

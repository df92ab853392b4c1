"""Checkpoint format.

The reference pickles the whole module (``torch.save(model)``, nmt_multimodal_beam_DE.py:491-520) and keeps no
optimiser state, so training cannot resume.  Here a checkpoint is a plain dict of tensors keyed by the reference's
parameter names -- loadable into the reference's own classes and vice versa -- plus, optionally, the fused optimiser's
state (Adam moments per parameter name, step counter, learning rate), the averaged weights of a driver that keeps them
(``ckpt["ema"]``: decay, warm-up flag, one tensor per parameter name) and the dropout generator's {seed, step} words.
Whole-module pickles keep working too (the modules hold no library handles)."""
import math
import warnings

import torch

FORMAT = "vag-nmt-checkpoint-v1"


def save_checkpoint(path, model, train_step=None, extra=None):
    if train_step is not None and getattr(train_step, "_averaged", False):
        raise RuntimeError("save_checkpoint with a driver inside averaged_weights(): the parameters are the averaged weights there "
                           "(torch.save(model) or ema_state_dict() export those)")
    ckpt = {"format": FORMAT,
            "state_dict": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
            "extra": extra or {}}
    rng = getattr(model, "_vag_rng", None)
    if rng is not None:
        ckpt["dropout_rng"] = rng.detach().cpu().clone()
    if train_step is not None:
        if hasattr(train_step, "check") and train_step.fp.flat.is_cuda:
            train_step.check()            # never write a checkpoint over steps the device had to skip without saying so
        if hasattr(train_step, "gather_optimizer_state"):
            train_step.gather_optimizer_state()      # (sharded optimiser: every rank's copy of the moments made whole first)
        fp = train_step.fp
        m, v = {}, {}
        for name, p in fp.named:
            o, k = fp.offsets[name], p.numel()
            m[name] = fp.m[o:o + k].view_as(p).detach().cpu().clone()
            v[name] = fp.v[o:o + k].view_as(p).detach().cpu().clone()
        ckpt["optimizer"] = {"kind": "adam", "m": m, "v": v, "step": int(train_step.step_count.item()),
                             "lr": train_step.lr, "betas": tuple(train_step.betas), "eps": train_step.eps,
                             "weight_decay": train_step.wd, "clip": train_step.clip}
        if getattr(fp, "ema", None) is not None:
            # the averaged weights, sliced per name like the moments (the slot padding is not state); "tied": the further names
            # model.state_dict() lists a tied tensor under, so that a reader without the model can form a whole state_dict
            from .trainer import tied_names
            e = {}
            for name, p in fp.named:
                o, k = fp.offsets[name], p.numel()
                e[name] = fp.ema[o:o + k].view_as(p).detach().cpu().clone()
            ckpt["ema"] = {"decay": train_step.ema_decay, "warmup": train_step.ema_warmup, "params": e,
                           "tied": tied_names(model, fp)}
    torch.save(ckpt, path)
    return ckpt


def _read(path, map_location):
    """(state_dict, checkpoint dict or {}) of any of the three accepted forms."""
    obj = torch.load(path, map_location=map_location, weights_only=False)
    if isinstance(obj, torch.nn.Module):
        return obj.state_dict(), {}
    if isinstance(obj, dict) and obj.get("format") == FORMAT:
        return obj["state_dict"], obj
    return obj, {}


def _averaged_state_dict(sd, ckpt, path):
    """The checkpoint's state_dict with the stored averaged weights in place of the raw parameters."""
    if "ema" not in ckpt:
        raise KeyError("%s holds no averaged weights (no 'ema' entry: written without TrainStep(ema_decay > 0))" % (path,))
    e = ckpt["ema"]
    out = dict(sd)
    out.update(e["params"])
    for alias, name in e.get("tied", {}).items():
        if alias in out:
            out[alias] = e["params"][name]
    return out


def load_checkpoint(path, model, train_step=None, map_location="cpu", use_ema=False):
    """Accepts this format, a bare state_dict (reference parameter names), or a pickled module.
    With a driver that averages (``TrainStep(ema_decay > 0)``) the stored average is copied in place into ``fp.ema``; a checkpoint
    that holds none starts the average at the loaded parameters and warns.  ``use_ema=True``: the averaged weights go into ``model``
    instead of the raw ones (decoding or export without a driver; with ``train_step`` it is a ValueError, on a checkpoint without
    an average a KeyError)."""
    if use_ema and train_step is not None:
        raise ValueError("use_ema=True loads the averaged weights as the model's parameters: not together with a train_step "
                         "(which restores both copies)")
    if train_step is not None and getattr(train_step, "_averaged", False):
        raise RuntimeError("load_checkpoint with a driver inside averaged_weights(): the two sets of weights have changed places there")
    sd, ckpt = _read(path, map_location)
    if use_ema:
        sd = _averaged_state_dict(sd, ckpt, path)
    missing, unexpected = model.load_state_dict(sd, strict=False)      # copies into the (possibly flat-buffer) views
    if unexpected or not set(missing) <= {"decoder.out.weight"}:
        raise RuntimeError("checkpoint does not match the model: missing %s unexpected %s" % (missing, unexpected))
    if "dropout_rng" in ckpt:
        # in place: captured step graphs hold the device address of these two words
        from .state import dropout_rng
        dropout_rng(model, next(model.parameters()).device).copy_(ckpt["dropout_rng"])
    if train_step is not None and "optimizer" in ckpt:
        opt, fp = ckpt["optimizer"], train_step.fp
        with torch.no_grad():
            for name, p in fp.named:
                o, k = fp.offsets[name], p.numel()
                fp.m[o:o + k].copy_(opt["m"][name].reshape(-1))
                fp.v[o:o + k].copy_(opt["v"][name].reshape(-1))
            train_step.step_count.fill_(int(opt["step"]))
        train_step.set_lr(opt["lr"])
    if train_step is not None and getattr(train_step.fp, "ema", None) is not None:
        fp = train_step.fp
        with torch.no_grad():                     # in place: captured graphs hold fp.ema's address
            if "ema" in ckpt:
                for name, p in fp.named:
                    o, k = fp.offsets[name], p.numel()
                    fp.ema[o:o + k].copy_(ckpt["ema"]["params"][name].reshape(-1))
            else:
                warnings.warn("%s holds no averaged weights: the average restarts from the loaded parameters" % (path,))
                fp.ema.copy_(fp.flat)
    if train_step is not None and hasattr(train_step.backend, "after_optimizer"):
        train_step.backend.after_optimizer()      # derived weights follow the restored parameters
    return ckpt


def average_checkpoints(paths, weights=None, use_ema=False, map_location="cpu"):
    """The (weighted) mean of the ``state_dict``s of several checkpoints, each in any form ``load_checkpoint`` accepts: the
    classical alternative to ``TrainStep(ema_decay > 0)`` for runs trained without it (average the last few checkpoints).
    Accumulated in fp64 in list order, returned as an fp32 ``state_dict`` (entries that are not floating point are taken from the
    first checkpoint and must agree).  ``use_ema=True`` averages the stored averaged weights instead (KeyError where a checkpoint
    holds none).  Names and shapes must agree; ``weights`` must be finite with a positive sum.  Plain torch on the CPU."""
    paths = list(paths)
    if not paths:
        raise ValueError("average_checkpoints needs at least one checkpoint")
    w = [1.0] * len(paths) if weights is None else [float(x) for x in weights]
    if len(w) != len(paths):
        raise ValueError("one weight per checkpoint (%d), got %d" % (len(paths), len(w)))
    if not all(math.isfinite(x) for x in w) or not sum(w) > 0.0:
        raise ValueError("weights must be finite and have a positive sum, got %r" % (w,))
    total = sum(w)
    acc, first = {}, None
    for path, wi in zip(paths, w):
        sd, ckpt = _read(path, map_location)
        if use_ema:
            sd = _averaged_state_dict(sd, ckpt, path)
        sd = {k: v.detach().cpu() for k, v in sd.items()}
        if first is None:
            first = sd
        elif set(sd) != set(first):
            raise ValueError("%s: parameter names differ from the first checkpoint's: %s" % (path, sorted(set(sd) ^ set(first))))
        for k, v in sd.items():
            if v.shape != first[k].shape or v.dtype.is_floating_point != first[k].dtype.is_floating_point:
                raise ValueError("%s: %s is %s %s, the first checkpoint has %s %s"
                                 % (path, k, tuple(v.shape), v.dtype, tuple(first[k].shape), first[k].dtype))
            if not v.dtype.is_floating_point:
                if not torch.equal(v, first[k]):
                    raise ValueError("%s: %s (not floating point) differs from the first checkpoint's" % (path, k))
                continue
            term = v.to(torch.float64) * (wi / total)
            acc[k] = term if k not in acc else acc[k] + term
    return {k: (acc[k].to(torch.float32) if k in acc else first[k].clone()) for k in first}

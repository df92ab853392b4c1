"""Sampling decoder: translations DRAWN from one model's or an ensemble's distribution (back-translation data, calibration
checks), with a temperature, an optional top-k cut and an optional nucleus (top-p) cut.

Every step is the search's member steps (vagnmt_hip.search) followed by ONE launch of vag_sample_step (csrc/sample.hip), which
scores each word as the ensemble search does, keeps the top_k best (0: all) and draws by Gumbel-max from a counter-based
generator.  A decode is a pure function of (inputs, generator state): the same state gives the same samples.

    gen = Generator(1234)
    out = model.sample_decode(src_var, src_lengths, im_var, n_samples=4, temperature=0.9, top_k=10, generator=gen)
    out.hyps[b][j]        sample j of sentence b, a token list cut at EOS
    out.token_logp        (B, n_samples, max_length): the model's own (untempered, untruncated) log-probability of each drawn
                          word, 0 after the first EOS -- what score_translations gives for the same words
    out.logp, out.score   (B, n_samples): their sum, and the sum / max(1, #words > 3): the beam search's length normalisation

Nucleus sampling: ``top_p`` in (0, 1] keeps, of the candidates (every word, or the top_k best), the best words that carry top_p
of their tempered mass -- whole groups of equal scores, see include/vag_nmt.h: vag_sample_step_p -- and draws among those; the
order is temperature, top_k, top_p.  ``return_sizes=True`` also returns how many words each draw chose from:

    out, sizes = model.sample_decode(src_var, src_lengths, im_var, n_samples=4, top_p=0.9, return_sizes=True, generator=gen)
    sizes                 (B, n_samples, max_length) int32, 0 after a sample's first EOS

top_p = 1.0 without sizes is the decode above, launch for launch.

With top_k = 0 every word is a candidate, the padding word 0 included (an untrained model draws it now and then, a trained one
hardly ever).  It is kept in hyps and counted in token_logp and logp; score_translations feeds such a word to the next step but
does not score its position, so its sums differ from these by exactly that word's log-probability.
"""
from collections import namedtuple

import numpy as np
import torch

from vagnmt_hip import search
from vagnmt_hip._lib import call, ptr, stream
from vagnmt_hip.search import EOS_token

MAX_TOP_K = 64          # the selection kernels rank at most 64 candidates (include/vag_nmt.h: vag_sample_step)

Sampled = namedtuple("Sampled", ["hyps", "token_logp", "logp", "score"])


class Generator:
    """The sampler's random state: {seed, call counter} as uint64[2] in device memory (the layout of the dropout generator),
    created on first use on the device that asks for it.  Every sampling call draws under the current state and then advances
    the counter on the device (vag_rng_advance); ``get_state`` / ``set_state`` copy it out and back to repeat a call."""

    def __init__(self, seed=0):
        seed = int(seed) % (1 << 64)
        self.seed = seed
        self._words = [seed - (1 << 64) if seed >= (1 << 63) else seed, 0]        # as int64 bit patterns
        self._state = None

    def state(self, device):
        if self._state is None or self._state.device != torch.device(device):
            if self._state is not None:
                self._words = [int(x) for x in self._state.cpu()]
            self._state = torch.tensor(self._words, dtype=torch.int64, device=device)
        return self._state

    def advance(self):
        call("vag_rng_advance", ptr(self._state, torch.int64), stream())

    def get_state(self):
        return [int(x) for x in self._state.cpu()] if self._state is not None else list(self._words)

    def set_state(self, words):
        self._words = [int(words[0]), int(words[1])]
        if self._state is not None:
            self._state.copy_(torch.tensor(self._words, dtype=torch.int64))


def default_generator(owner):
    """The generator a model or an ensemble uses when none is given: one per object, seeded from torch.initial_seed().  Kept
    under a ``_decode_`` name: a whole-module pickle does not carry it."""
    gen = owner.__dict__.get("_decode_generator")
    if gen is None:
        gen = owner.__dict__["_decode_generator"] = Generator(torch.initial_seed())
    return gen


def check_args(src_var, n_samples, max_length, temperature, top_k, what="sample_decode"):
    """Host-side checks of sample_decode; returns (n_samples, max_length, temperature, top_k) as plain numbers."""
    n, ml, k = int(n_samples), int(max_length), int(top_k)
    t = float(temperature)
    if n < 1:
        raise ValueError("%s: n_samples must be at least 1, got %d" % (what, n))
    if ml < 1:
        raise ValueError("%s: max_length must be at least 1, got %d" % (what, ml))
    if not (t > 0.0 and t < float("inf")):
        raise ValueError("%s: temperature must be positive and finite, got %r" % (what, temperature))
    if not (0 <= k <= MAX_TOP_K):
        raise ValueError("%s: top_k must be 0 (the whole vocabulary) or 1 .. %d, got %d" % (what, MAX_TOP_K, k))
    if not torch.is_tensor(src_var) or not src_var.is_cuda:
        raise ValueError("%s: src_var must be a GPU tensor (there is no CPU path)" % what)
    return n, ml, t, k


def check_top_p(top_p, what="sample_decode"):
    """top_p of sample_decode as a plain number: in (0, 1], not NaN."""
    p = float(top_p)
    if not (p > 0.0 and p <= 1.0):
        raise ValueError("%s: top_p must be in (0, 1], got %r" % (what, top_p))
    return p


def nucleus_key(top_p, return_sizes):
    """What a nucleus decode adds to (temperature, top_k) in the key of its decode state: () for top_p = 1 without sizes, which
    is the plain sampling decode and shares its state and captured graphs."""
    return () if top_p == 1.0 and not return_sizes else (top_p, bool(return_sizes))


def assemble_sizes(sizes, B, n, device=None):
    """The nucleus sizes of a decode, (L, B n) int32 time-major as vag_sample_step_p writes them -> (B, n, L)."""
    return sizes.t().reshape(B, n, -1).contiguous().to(device)


def assemble(toks, lps, B, n, device=None):
    """The history of a sampling decode -> Sampled.  toks (L, B n) int64 and lps (L, B n) float32, time-major rows as
    vag_sample_step writes them (arrays or tensors).  Each sample spans up to and including its first EOS (everything, if there
    is none): hyps[b][j] is cut before it, token_logp (B, n, L) is 0 after it, logp adds the span in position order in float32
    and score = logp / max(1, #words > 3 in the span), vag_forced_score's form of vag_beam_finish's normalisation."""
    toks = np.asarray(toks.cpu() if torch.is_tensor(toks) else toks).astype(np.int64).T                  # (N, L)
    lps = np.asarray(lps.cpu() if torch.is_tensor(lps) else lps).astype(np.float32).T
    N, L = toks.shape
    assert N == B * n, (N, B, n)
    ended = np.cumsum(toks == EOS_token, axis=1) - (toks == EOS_token)           # EOS seen strictly before this position
    span = ended == 0
    token_logp = np.where(span, lps, np.float32(0)).astype(np.float32)
    logp = np.cumsum(token_logp, axis=1, dtype=np.float32)[:, -1]
    words = np.maximum(1, ((toks > 3) & span).sum(1)).astype(np.float32)
    score = (logp / words).astype(np.float32)
    hyps = []
    for b in range(B):
        rows = []
        for j in range(n):
            r = toks[b * n + j]
            stop = np.nonzero(r == EOS_token)[0]
            rows.append([int(t) for t in (r[:stop[0]] if len(stop) else r)])
        hyps.append(rows)
    return Sampled(hyps, torch.from_numpy(token_logp.reshape(B, n, L)).to(device),
                   torch.from_numpy(logp.reshape(B, n).copy()).to(device), torch.from_numpy(score.reshape(B, n)).to(device))


def sample_history(obj, src_var, src_lengths, im_var, n_samples, max_length, temperature, top_k, generator, top_p, return_sizes,
                   what="sample_decode"):
    """The draws of sample_decode / mbr_decode / mrt_step on a model or an Ensemble: search.sample on its members (the plain, not
    hoisted, steps in both modes), the generator (None: the object's own) advanced once.  Returns the sampler's time-major history
    on the device, (toks, lps, sizes or None, B, n).  Key fragment ("sample", temperature, top_k) + nucleus_key: by-value
    arguments of the captured launches; top_p = 1.0 without sizes is the plain sampling decode, state key and launches."""
    p = check_top_p(top_p, what)
    n, ml, t, k = check_args(src_var, n_samples, max_length, temperature, top_k, what)
    gen = generator if generator is not None else default_generator(obj)
    with torch.no_grad():
        s = obj._search_setup(src_var, src_lengths, im_var, n, ml, "sample", hoist=False,
                              extra=("sample", t, k) + nucleus_key(p, return_sizes), what=what)
        sizes = torch.empty(ml, s.B * n, dtype=torch.int32, device=s.device) if return_sizes else None
        toks, lps, obj.last_decode_steps = search.sample(s.members, s.h0s, n, ml, t, k, gen.state(s.device), s.entry, s.pool,
                                                         top_p=p, sizes=sizes)
        gen.advance()
    return toks, lps, sizes, s.B, n


def sample_decode(obj, src_var, src_lengths, im_var, n_samples, max_length, temperature, top_k, generator, top_p=1.0,
                  return_sizes=False):
    """sample_decode of a model or an Ensemble -> Sampled, or (Sampled, sizes) with return_sizes."""
    toks, lps, sizes, B, n = sample_history(obj, src_var, src_lengths, im_var, n_samples, max_length, temperature, top_k, generator,
                                            top_p, return_sizes)
    out = assemble(toks, lps, B, n, toks.device)
    return (out, assemble_sizes(sizes, B, n)) if return_sizes else out

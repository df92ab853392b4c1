"""What every public decoding method of a model and of an Ensemble hands to vagnmt_hip.search, pinned to
tests/golden/decode_dispatch.json: the layer between the public methods and the search functions may be rearranged, but a
rearrangement must not change which search runs, its arguments, the decode states and entries it runs on (their cache keys,
element for element), the steps the members run (hoisted or plain), or what is set on the object afterwards.

No device.  The members are tiny CPU models -- one multimodal, one text-only -- and an Ensemble of both.  ``_decode_prologue``
returns fixed tensors, plain ones (eager mode) or ones that report ``is_cuda`` (graph mode); the search functions, the operators a
Member and a decode state call, ``Generator.advance`` and the selection of mbr_decode are replaced.  The library itself is loaded
for size queries only.  Recorded per call of a search function: its name and arguments (bound to its signature, defaults filled
in: a scalar by value, a hook object by class and public scalar fields, a tensor or array by shape and dtype), per member its
model, whether its steps are the hoisted ones and whether it keeps attention rows, which dict the entry is and which pool.
Recorded per case: those calls, the keys the case added to the models' decode caches and to the Ensemble's cache (weight
pointers, store / language-model pointers and member identities replaced by tags), last_decode_steps, last_beam_scores,
beam_size, the generator's advances and the result's type.

The golden file was written by this module's __main__ against the commit before the variants moved into their feature modules:
    python tests/test_decode_dispatch_host.py --pkg <checkout>/vag-nmt_amd --out tests/golden/decode_dispatch.json"""
import inspect
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

B, TS, ML, VS, VT, IM = 2, 5, 6, 30, 40, 24
HS = (16, 8)                     # hidden sizes of the multimodal and the text-only member
SEARCHES = ("greedy", "beam", "beam_diverse", "beam_required", "beam_stochastic", "beam_penalised", "sample")


class FakeCuda(torch.Tensor):
    """A CPU tensor that reports is_cuda: what the host layer looks at to choose graph mode and to accept its inputs."""
    is_cuda = property(lambda self: True)


def fake(t):
    return t.as_subclass(FakeCuda)


def plain(x):
    """JSON form of an argument: scalars by value, tensors / arrays by shape and dtype, hooks by class and scalar fields."""
    if isinstance(x, (bool, int, str)) or x is None:
        return "ptr" if isinstance(x, int) and not isinstance(x, bool) and abs(x) >= 1 << 32 else x
    if isinstance(x, float):
        return repr(x)
    if torch.is_tensor(x):
        return "tensor:%s%s" % (str(x.dtype).replace("torch.", ""), list(x.shape))
    if isinstance(x, np.ndarray):
        return "array:%s%s" % (x.dtype, list(x.shape))
    if isinstance(x, (list, tuple)):
        return [plain(y) for y in x]
    fields = {k: plain(v) for k, v in sorted(vars(x).items())
              if not k.startswith("_") and isinstance(v, (bool, int, float, str))}
    return {"class": type(x).__name__, **fields}


class FakeLM:
    """Stands for an NgramLM: the search only keeps it and asks for its identity."""
    V = VT

    def identity(self):
        return (1 << 40, 3, VT)


class World:
    """The package under test with its device side replaced, two models, their Ensemble and the record of one case."""

    def __init__(self):
        from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11, NMT_Seq2Seq_Beam_V2
        from vagnmt_hip import _lib, knn, lm, mbr, mrt, ops, sampling, search
        from vagnmt_hip.ensemble import Ensemble
        self.search, self.knn, self.lm, self.mrt, self.sampling = search, knn, lm, mrt, sampling
        torch.manual_seed(0)
        mm = NMT_AttentionImagine_Seq2Seq_Beam_V11(VS, VT, IM, 8, 8, HS[0], 12, 0.99).eval()
        text = NMT_Seq2Seq_Beam_V2(VS, VT, 8, 8, HS[1]).eval()
        self.models = [mm, text]
        self.objects = {"mm": mm, "text": text, "ens": Ensemble(self.models)}
        self.graph = False
        self.calls, self.advances = [], 0
        self.saved = []

        def patch(owner, name, value):
            self.saved.append((owner, name, owner.__dict__.get(name, None), name in owner.__dict__))
            setattr(owner, name, value)

        for i, m in enumerate(self.models):
            patch(m, "_decode_prologue", self._prologue(i))
        for name in SEARCHES:
            patch(search, name, self._search_stub(name, getattr(search, name)))
        prep = lambda emb, dp: torch.zeros(_lib.lib().vag_cgru_prep_floats(dp[1].shape[1]))             # noqa: E731
        patch(ops, "decode_prepare", prep)
        patch(ops, "decode_tables", lambda emb, dp, hp, out=None: out if out is not None else torch.zeros(4))
        patch(ops, "decode_keys", lambda enc, prep, hp, out=None: out if out is not None else torch.zeros(4))
        patch(ops, "decode_hoisted_ok", lambda rows, emb, dp, hp: True)
        patch(ops, "greedy_decode_supported", lambda *a: False)
        patch(ops, "KeysProj", types.SimpleNamespace(apply=lambda enc, w: torch.zeros(enc.shape)))
        patch(sampling.Generator, "advance", lambda gen: setattr(self, "advances", self.advances + 1))
        patch(lm, "check_lm", lambda model, models, device, what: model)
        patch(mbr, "_run", lambda hyps, refs, weights, uid, surface: (torch.zeros(hyps.shape[0], dtype=torch.int64),
                                                                      torch.zeros(hyps.shape[0], hyps.shape[1])))
        patch(mbr, "select_args", lambda hyps, refs=None, weights=None, utility="bleu", surface=None: (hyps, refs, weights, 0))
        self.stores = []
        for h in HS:
            s = knn.Datastore(h, "cpu")
            s._chunks = [dict(keys=torch.zeros(7, h, dtype=torch.bfloat16), norm=torch.zeros(7),
                              values=torch.arange(4, 11, dtype=torch.int32), sentence=torch.zeros(7, dtype=torch.int32),
                              position=torch.zeros(7, dtype=torch.int32))]
            s._fill = s._n = 7
            self.stores.append(s)

    def close(self):
        for owner, name, old, had in reversed(self.saved):
            if had:
                setattr(owner, name, old)
            else:
                delattr(owner, name)

    # ---------------------------------------------------------------------------------------------------- the replacements
    def _prologue(self, i):
        def prologue(src_var, src_lengths, im_var):
            out = (torch.zeros(B, TS, 2 * HS[i]), torch.ones(B, TS), torch.zeros(B, HS[i]))
            return tuple(fake(t) for t in out) if self.graph else out
        return prologue

    def _member(self, mb):
        return {"model": [i for i, m in enumerate(self.models) if m.decoder.embedding.weight is mb.emb][0],
                "hoisted": bool(mb.hoisted), "align": bool(mb.align), "graph": mb.st is not None}

    def _entry(self, entry, members):
        if entry is None:
            return None
        if len(members) == 1 and entry is members[0].st:
            return "member state"
        ens = self.objects["ens"]
        return "ensemble entry" if any(v is entry for v in ens._cache.values()) else "?"

    def _search_stub(self, name, real):
        sig = inspect.signature(real)

        def stub(*args, **kw):
            ba = sig.bind(*args, **kw)
            ba.apply_defaults()
            a = dict(ba.arguments)
            members = a.pop("members")
            rec = {"search": name, "members": [self._member(mb) for mb in members],
                   "h0s": plain(a.pop("h0s")), "entry": self._entry(a.pop("entry"), members)}
            pool = a.pop("pool")
            rec["pool"] = None if pool is None else "%s.%s" % (type(pool.__self__).__name__, pool.__name__)
            rec["args"] = {k: plain(v) for k, v in a.items()}
            self.calls.append(rec)
            return self._result(name, a)
        return stub

    def _result(self, name, a):
        """What the search would return, in shape: enough for the feature modules' assembling code to run on it."""
        hyps = lambda n: [[[5, 6]] * n for _ in range(B)]              # noqa: E731
        f = lambda *shape: torch.zeros(*shape)                         # noqa: E731
        i64 = lambda *shape: torch.zeros(*shape, dtype=torch.int64)    # noqa: E731
        if name == "greedy":
            return i64(B, a["tgt_l"]) if a["device_rows"] else [[5, 6]] * B
        k, ml = a.get("k"), a["max_length"]
        if name == "sample":
            n = a["n"]
            if a["sizes"] is not None:
                a["sizes"].zero_()
            return i64(ml, B * n) + 5, f(ml, B * n), 3
        n = a.get("n_best") or k
        if name == "beam":
            if a["align"]:
                return (hyps(n), f(B, n), f(B, n, ml, TS), i64(B, n, ml)), f(B), 4
            if a["n_best"]:
                return (hyps(n), f(B, n)), f(B), 4
            return (i64(B, ml) if a["device_rows"] else [[5, 6]] * B), f(B), 4
        if name == "beam_diverse":
            return (hyps(n), f(B, n), i64(B, n)), f(B), 4
        if name == "beam_required":
            return (hyps(n), f(B, n), i64(B, n), torch.zeros(B, k, 4, dtype=torch.int32)), f(B), 4
        if name == "beam_stochastic":
            return (hyps(k), i64(B, k, ml) + 5, f(B, k), f(B, k), -torch.arange(k).float().repeat(B, 1), f(B, 1)), f(B), 4
        return (hyps(n), f(B, n), f(B, n), torch.zeros(B, n, dtype=torch.int32), f(B, n)), f(B), 4

    # -------------------------------------------------------------------------------------------------------- one case
    def _keys(self):
        """The cache keys of the models (weight pointers -> "w") and of the Ensemble (member identities -> "m")."""
        out = {}
        for i, m in enumerate(self.models):
            nw = len(m.decoder.dec_params()) + len(m.decoder.head_params()) + 2
            out["model%d" % i] = sorted(json.dumps(plain(key[:-nw]) + ["w"]) for key in m.__dict__.get("_decode_cache", {})
                                        if key != "__pool__")
        ens = self.objects["ens"]
        out["ens"] = sorted(json.dumps(plain(key[:-len(self.models)]) + ["m"]) for key in ens._cache if key != "__pool__")
        return out

    def run(self, who, graph, call):
        obj = self.objects[who]
        self.graph, self.calls, self.advances = graph, [], 0
        for o in list(self.objects.values()):
            o.decode_graph = True
            for name in ("last_decode_steps", "last_beam_scores", "_decode_cache", "_decode_wcache", "_decode_generator"):
                o.__dict__.pop(name, None)
            o.beam_size = "unset"
        self.objects["ens"]._cache.clear()
        src = fake(torch.full((B, TS), 4, dtype=torch.int64))
        res = call(self, obj, who, src, [TS] * B, torch.zeros(B, IM))
        kinds = res if isinstance(res, str) else \
            [type(r).__name__ for r in res] if type(res) in (tuple, list) else type(res).__name__
        return {"calls": self.calls, "keys": self._keys(), "steps": plain(getattr(obj, "last_decode_steps", "unset")),
                "scores": plain(getattr(obj, "last_beam_scores", "unset")), "beam_size": plain(obj.beam_size),
                "advances": self.advances, "result": kinds}


def _im(who, im, *rest):
    """Positional arguments after (src_var, src_lengths): the text-only model's reference signatures take no im_var."""
    return rest if who == "text" else (im,) + rest


def _cases():
    c = {}
    for k in (1, 3):
        c["decode_k%d" % k] = lambda w, o, who, s, l, im, k=k: o.beamsearch_decode(s, l, *_im(who, im, k, ML))
    c["nbest"] = lambda w, o, who, s, l, im: o.beamsearch_nbest(s, l, *_im(who, im, 4, 2, ML, False, True))
    c["align"] = lambda w, o, who, s, l, im: o.beamsearch_align(s, l, *_im(who, im, 4, 2, ML))
    c["diverse"] = lambda w, o, who, s, l, im: o.beamsearch_diverse(s, l, im, beam_size=4, n_groups=2, diversity=0.5, max_length=ML)
    for n in (0, 3):
        c["constrained_ngram%d" % n] = lambda w, o, who, s, l, im, n=n: o.beamsearch_constrained(
            s, l, *_im(who, im), beam_size=4, n_best=2, max_length=ML, prefix=[[7], []], banned=[[9, 10]], no_repeat_ngram=n)
    c["required"] = lambda w, o, who, s, l, im: o.beamsearch_required(s, l, im, 4, 2, ML, required=[[[7, 8]], []])
    c["required_negative"] = lambda w, o, who, s, l, im: o.beamsearch_required(s, l, im, 4, 2, ML, required=[[[7, 8]], []],
                                                                            banned=[[9]], no_repeat_ngram=2)
    for beta in (0.0, 0.2):
        for n in (0, 2):
            c["penalised_beta%s_ngram%d" % (beta, n)] = lambda w, o, who, s, l, im, beta=beta, n=n: o.beamsearch_penalised(
                s, l, im, 4, 2, ML, "gnmt", 0.6, beta, 0.1, True, no_repeat_ngram=n)
    c["stochastic"] = lambda w, o, who, s, l, im: o.beamsearch_stochastic(s, l, im, 4, ML, w.sampling.Generator(3))
    c["sample"] = lambda w, o, who, s, l, im: o.sample_decode(s, l, im, 3, ML, 0.9, 5)
    c["sample_top_p"] = lambda w, o, who, s, l, im: o.sample_decode(s, l, im, 3, ML, top_p=0.8)
    c["sample_sizes"] = lambda w, o, who, s, l, im: o.sample_decode(s, l, im, 3, ML, return_sizes=True)
    c["mbr"] = lambda w, o, who, s, l, im: o.mbr_decode(s, l, im, 4, ML)
    c["mbr_beam"] = lambda w, o, who, s, l, im: o.mbr_decode(s, l, im, 4, ML, beam_size=4)
    c["mbr_groups"] = lambda w, o, who, s, l, im: o.mbr_decode(s, l, im, 4, ML, beam_size=4, beam_groups=2)
    c["mbr_without_replacement"] = lambda w, o, who, s, l, im: o.mbr_decode(s, l, im, 4, ML, beam_size=2, without_replacement=True)
    stores = lambda w, who: w.stores if who == "ens" else w.stores[0] if who == "mm" else w.stores[1]      # noqa: E731
    con = dict(banned=[[9]], no_repeat_ngram=2)
    for tag, lam, kw in (("lam0", 0.0, {}), ("lam", 0.25, {}), ("lam_constrained", 0.25, con), ("lam0_constrained", 0.0, con)):
        c["knn_" + tag] = lambda w, o, who, s, l, im, lam=lam, kw=kw: o.beamsearch_knn(
            s, l, im, stores(w, who), 4, 2, ML, k=3, temperature=5.0, lam=lam, **kw)
        c["lm_" + tag.replace("lam", "beta")] = lambda w, o, who, s, l, im, lam=lam, kw=kw: o.beamsearch_lm(
            s, l, im, FakeLM(), lam, 4, 2, ML, **kw)

    def mrt_draw(method):
        def call(w, o, who, s, l, im):
            if who == "ens":
                return "not a TrainStep"
            return w.mrt._draw(types.SimpleNamespace(model=o), s, l, None if who == "text" else im, 3, ML, method, None)
        return call
    c["mrt_draw_stochastic"], c["mrt_draw_sample"] = mrt_draw("stochastic"), mrt_draw("sample")
    return c


def all_records():
    w = World()
    try:
        return {"%s/%s/%s" % (name, who, "graph" if graph else "eager"): w.run(who, graph, call)
                for name, call in _cases().items() for who in ("mm", "text", "ens") for graph in (False, True)}
    finally:
        w.close()


def intern(records):
    """The golden file's form: every distinct call / key text once, the cases as indices into that table."""
    table, index = [], {}

    def code(x):
        x = json.dumps(x, sort_keys=True)
        if x not in index:
            index[x] = len(table)
            table.append(x)
        return index[x]

    cases = {name: dict(r, calls=[code(x) for x in r["calls"]], keys=code(r["keys"])) for name, r in records.items()}
    return {"shapes": dict(B=B, Ts=TS, max_length=ML, V=VT, H=list(HS)), "table": table, "cases": cases}


def expand(golden):
    table = [json.loads(x) for x in golden["table"]]
    return {name: dict(r, calls=[table[i] for i in r["calls"]], keys=table[r["keys"]]) for name, r in golden["cases"].items()}


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_dispatch.json")


@pytest.fixture(scope="module")
def recorded():
    return json.loads(json.dumps(all_records()))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return expand(json.load(f))


def test_the_cases_are_the_golden_file_s(recorded, golden):
    assert sorted(recorded) == sorted(golden)
    assert len(recorded) == len(_cases()) * 6


@pytest.mark.parametrize("name", sorted(_cases()))
def test_dispatch_is_what_it_was(recorded, golden, name):
    for who in ("mm", "text", "ens"):
        for mode in ("eager", "graph"):
            case = "%s/%s/%s" % (name, who, mode)
            got, want = recorded[case], golden[case]
            assert len(got["calls"]) == len(want["calls"]), case
            for g, w in zip(got["calls"], want["calls"]):
                assert g == w, case
            assert got == want, case


def test_the_record_sees_what_it_should(recorded):
    """The recorder itself: graph mode makes states and entries, eager mode none; lam = 0 runs the plain search on the plain
    search's state; sampling runs the plain steps, the beam searches the hoisted ones."""
    r = recorded["knn_lam0/mm/graph"]
    assert r["calls"][0]["search"] == "beam" and r["calls"][0]["args"]["knn"] is None and r["calls"][0]["entry"] == "member state"
    assert all(json.loads(k)[0] == "beam" for k in r["keys"]["model0"]) and r["beam_size"] == 4
    assert recorded["knn_lam/ens/graph"]["calls"][0]["entry"] == "ensemble entry"
    assert recorded["knn_lam/ens/eager"]["calls"][0]["entry"] is None and recorded["knn_lam/ens/eager"]["keys"]["ens"] == []
    assert [m["hoisted"] for m in recorded["sample/ens/graph"]["calls"][0]["members"]] == [False, False]
    assert [m["hoisted"] for m in recorded["diverse/ens/eager"]["calls"][0]["members"]] == [True, True]
    assert recorded["sample/mm/eager"]["advances"] == 1 and recorded["mbr_beam/mm/eager"]["advances"] == 1
    assert "constrain" in json.loads(recorded["required_negative/text/graph"]["keys"]["model1"][0])


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", required=True, help="the vag-nmt_amd directory whose decoding layer is recorded")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    import vagnmt_hip
    assert os.path.abspath(vagnmt_hip.__file__).startswith(os.path.abspath(a.pkg)), vagnmt_hip.__file__
    g = intern(json.loads(json.dumps(all_records())))
    with open(a.out, "w") as f:
        json.dump(g, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d cases, %d distinct records -> %s" % (len(g["cases"]), len(g["table"]), a.out))

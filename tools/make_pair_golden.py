"""Golden vectors of the pairwise interaction helpers (cosine_distance, l1_distance, moving_average, _get_doc_context_copacrr,
layers.MovingAverage, MatchingHistogram), captured from the upstream reference in the build container -- never on the GPU
machine, and no test reads the reference.

``torch_utils.py``, ``layers.py`` and ``matchzoo/preprocessors/units/matching_histogram.py`` are loaded by path
(golden_common.load_reference).  ``torch_utils.py`` imports torchvision, which the container does not have: an empty stub
module stands in for it.  ``matching_histogram.py`` imports ``.unit`` relatively, so ``units/unit.py`` is loaded first under a
synthetic package name; the ``matchzoo`` package and its data pipeline are never imported.  The generator writes

    tests/golden/g20_pair.npz           every case below; ``meta`` lists the cases and their parameters

Per case ``<family>::<name>::``:
  ``l2`` / ``l1``  (cosine_distance / l1_distance) at (B, L, R, D): s5x3 (2,5,3,6), s21x9 (3,21,9,10), s37x35 (2,37,35,70),
      s19x20 (1,19,20,700): ``a``, ``b``, ``g``, ``out``, ``grad::a``, ``grad::b``.
  ``ma``  (moving_average(x, w, 1)) at (B, L, D, w): w1 (2,7,6,1), wL (2,7,6,7), w3 (3,21,10,3), w5 (2,100,30,5),
      long (1,1024,8,64), over (2,3,4,5: the window is longer than the sequence, the result is (B,0,D));
      ``mod`` (layers.MovingAverage(w, 1)) at w2 (3,9,5,2): ``x``, ``g``, ``out``, ``grad::x``.
  ``ctx``  (_get_doc_context_copacrr(doc, mask, c)) at (B, L, D, c): c2 (3,9,5,2), c3 (3,21,10,3), c4 (2,100,30,4),
      c5 (3,100,30,5), with masks built from lengths that include a full and (c3, c5) an all-masked sequence: ``x``, ``mask``,
      ``g``, ``out``, ``grad::x``.
  ``hist``  (MatchingHistogram(bins, table, normalize, mode).transform per sample, the right ids cut at ``len_right`` as
      data_generator/callbacks/histogram.py does) at (V, D, Lq, Ld, bins): n300 (50,300,5,40,30), n10 (40,10,7,33,30),
      n6 (30,6,3,5,3) with normalize=True and the two sides drawn from disjoint halves of the vocabulary; shared (20,8,4,9,30),
      normalize=True, both sides from the whole vocabulary; dyadic (33,4,6,21,30), normalize=False, a table of entries k/8,
      |k| <= 4, whose every product is a multiple of 1/64 in [-1, 1].  Three samples each.  ``table``, ``ids_left``,
      ``ids_right``, ``len_right``, ``scaled`` (float64 (B,Lq,Ld): the reference's own (v + 1) / 2 (bins - 1) from its
      normalised table, NaN beyond len_right) and ``out::CH`` / ``out::NH`` / ``out::LCH``.

Inputs are 0.7 randn (tables: randn) rounded to what float16 holds exactly and stored as float16.  Upstream gradients are
randint(-16, 17) / 16.  Every differentiable case runs in fp32 and in float64; the stored results are the fp32 ones, and the
reference's own fp32 result must lie within one tenth of the bound the tests apply: 1e-4 of the largest float64 entry of the
tensor.

    python tools/make_pair_golden.py
"""
import json
import os
import sys
import types
import zlib
from unittest import mock

import numpy as np
import torch

from golden_common import OUT, load_reference, margin, to_numpy, write_npz

PAIR_SHAPES = {"s5x3": (2, 5, 3, 6), "s21x9": (3, 21, 9, 10), "s37x35": (2, 37, 35, 70), "s19x20": (1, 19, 20, 700)}
MA_SHAPES = {"w1": (2, 7, 6, 1), "wL": (2, 7, 6, 7), "w3": (3, 21, 10, 3), "w5": (2, 100, 30, 5), "long": (1, 1024, 8, 64),
             "over": (2, 3, 4, 5)}
MOD_SHAPES = {"w2": (3, 9, 5, 2)}
CTX_SHAPES = {"c2": (3, 9, 5, 2), "c3": (3, 21, 10, 3), "c4": (2, 100, 30, 4), "c5": (3, 100, 30, 5)}
CTX_LENS = {"c2": [9, 4, 1], "c3": [21, 0, 10], "c4": [100, 37], "c5": [63, 100, 0]}
HIST = {"n300": (50, 300, 5, 40, 30, True, "halves"), "n10": (40, 10, 7, 33, 30, True, "halves"), "n6": (30, 6, 3, 5, 3, True, "halves"),
        "shared": (20, 8, 4, 9, 30, True, "whole"), "dyadic": (33, 4, 6, 21, 30, False, "whole")}
HIST_LENS = {"n300": [40, 17, 1], "n10": [33, 16, 0], "n6": [5, 2, 4], "shared": [9, 5, 7], "dyadic": [21, 16, 3]}
HIST_MODES = ("CH", "NH", "LCH")
TOL_MAX = 1e-4


def half_exact(t):
    return t.half().float()


def upstream(g, shape):
    return torch.randint(-16, 17, tuple(shape), generator=g).float() / 16


def gen_for(key):
    return torch.Generator().manual_seed(zlib.crc32(key.encode()) ^ 0x5EED)


def store_half(res, name, t):
    res[name] = t.numpy().astype(np.float16)
    assert np.array_equal(res[name].astype(np.float32), t.numpy()), name


def run_diff(fn, inputs, key, dtype, extra=()):
    """fn(*differentiable inputs, *extra) in `dtype`, its gradient under the case's upstream gradient."""
    args = [t.to(dtype).clone().requires_grad_(True) for _, t in inputs]
    out = fn(*args, *extra)
    g = upstream(torch.Generator().manual_seed(zlib.crc32(key.encode()) ^ 0xC0FFEE), out.shape)
    if out.numel():
        (out * g.to(dtype)).sum().backward()
    res = {"out": out}
    store_half(res, "g", g)
    for (name, t), a in zip(inputs, args):
        store_half(res, name, t)
        res["grad::" + name] = a.grad if a.grad is not None else torch.zeros_like(a)
    return to_numpy(res)


def differentiable_cases(ref):
    """(key, function, [(name, tensor)], extra arguments, arrays to store next to the results, meta)."""
    for name, (B, L, R, D) in PAIR_SHAPES.items():
        for fam, fn in (("l2", ref["cosine_distance"]), ("l1", ref["l1_distance"])):
            key = f"{fam}::{name}"
            g = gen_for(f"pair::{name}")          # l2 and l1 run on the same inputs
            a, b = half_exact(0.7 * torch.randn(B, L, D, generator=g)), half_exact(0.7 * torch.randn(B, R, D, generator=g))
            yield key, fn, [("a", a), ("b", b)], (), {}, {"shape": [B, L, R, D]}
    for fam, shapes in (("ma", MA_SHAPES), ("mod", MOD_SHAPES)):
        for name, (B, L, D, w) in shapes.items():
            key = f"{fam}::{name}"
            x = half_exact(0.7 * torch.randn(B, L, D, generator=gen_for(key)))
            fn = (lambda t, w=w: ref["moving_average"](t, w, 1)) if fam == "ma" else (lambda t, w=w: ref["MovingAverage"](w, 1)(t))
            yield key, fn, [("x", x)], (), {}, {"shape": [B, L, D], "window": w}
    for name, (B, L, D, c) in CTX_SHAPES.items():
        key = f"ctx::{name}"
        x = half_exact(0.7 * torch.randn(B, L, D, generator=gen_for(key)))
        lens = CTX_LENS[name]
        assert len(lens) == B and max(lens) == L
        mask = (torch.arange(L)[None, :] < torch.tensor(lens)[:, None]).to(torch.int64)
        yield (key, lambda t, m, c=c: ref["_get_doc_context_copacrr"](t, m, c), [("x", x)], (mask,),
               {"mask": mask.numpy().astype(np.uint8)}, {"shape": [B, L, D], "window": c, "lens": lens})


def hist_case(ref, name):
    V, D, Lq, Ld, bins, normalize, draw = HIST[name]
    key = f"hist::{name}"
    g = gen_for(key)
    lens = HIST_LENS[name]
    B = len(lens)
    if name == "dyadic":
        table = torch.randint(-4, 5, (V, D), generator=g).float() / 8
    else:
        table = half_exact(torch.randn(V, D, generator=g))
    if draw == "halves":
        ids_left = torch.randint(0, V // 2, (B, Lq), generator=g)
        ids_right = torch.randint(V // 2, V, (B, Ld), generator=g)
    else:
        ids_left = torch.randint(0, V, (B, Lq), generator=g)
        ids_right = torch.randint(0, V, (B, Ld), generator=g)
        if name == "shared":          # every left word occurs on the right of its sample, inside its length
            for i in range(B):
                ids_right[i, :min(Lq, lens[i])] = ids_left[i, :min(Lq, lens[i])]
    res = {"ids_left": ids_left.numpy().astype(np.int32), "ids_right": ids_right.numpy().astype(np.int32),
           "len_right": np.array(lens, np.int32)}
    store_half(res, "table", table)
    emb = table.double().numpy()
    scaled = np.full((B, Lq, Ld), np.nan, np.float64)
    for mode in HIST_MODES:
        unit = ref["MatchingHistogram"](bins, emb.copy(), normalize, mode)
        outs = []
        for i in range(B):
            left, right = ids_left[i].tolist(), ids_right[i].tolist()[:lens[i]]        # callbacks/histogram.py: _trunc_text
            outs.append(np.asarray(unit.transform([left, right]), dtype=np.float32).reshape(Lq, bins))
            e = unit._embedding_matrix
            if lens[i]:
                scaled[i, :, :lens[i]] = (e[left].dot(np.transpose(e[right])) + 1.) / 2. * (bins - 1.)
        res["out::" + mode] = np.stack(outs)
    res["scaled"] = scaled
    meta = {"shape": [V, D, Lq, Ld], "bins": bins, "normalize": normalize, "draw": draw, "lens": lens}
    return key, res, meta


def main():
    if "torchvision" not in sys.modules:          # torch_utils.py:8-9 import it; nothing these cases run touches it
        stub = types.ModuleType("torchvision")    # empty but for `transforms`, of which the module builds a pipeline when it loads
        stub.transforms = mock.MagicMock(name="torchvision.transforms")
        sys.modules["torchvision"] = stub
    tu = load_reference("torch_utils.py", "_ref_torch_utils")
    layers = load_reference("layers.py", "_ref_layers")
    pkg = types.ModuleType("_ref_units")          # the package matching_histogram.py's `from .unit import Unit` resolves in
    pkg.__path__ = []
    sys.modules["_ref_units"] = pkg
    units = os.path.join("matchzoo", "preprocessors", "units")
    unit = load_reference(os.path.join(units, "unit.py"), "_ref_units.unit")
    sys.modules["_ref_units.unit"] = unit
    mh = load_reference(os.path.join(units, "matching_histogram.py"), "_ref_units.matching_histogram")
    ref = {"cosine_distance": tu.cosine_distance, "l1_distance": tu.l1_distance, "moving_average": tu.moving_average,
           "_get_doc_context_copacrr": tu._get_doc_context_copacrr, "MovingAverage": layers.MovingAverage,
           "MatchingHistogram": mh.MatchingHistogram}
    torch.set_num_threads(1)
    store, cases, params = {}, [], {}
    bound = lambda k, want: TOL_MAX * max(np.abs(want).max() if want.size else 0.0, 1e-30)
    for key, fn, inputs, extra, arrays, meta in differentiable_cases(ref):
        r32 = run_diff(fn, inputs, key, torch.float32, extra)
        r64 = run_diff(fn, inputs, key, torch.float64, extra)
        keys = [k for k in r32 if k == "out" or k.startswith("grad::")]
        assert all(r32[k].dtype == np.float32 and r64[k].dtype == np.float64 for k in keys), key
        worst = margin(r32, r64, [k for k in keys if r64[k].size], bound)
        print(f"{key}: fp32 reference at {worst:.4f} of a tenth of the bound")
        assert worst <= 1.0, (key, worst)
        assert all(np.isfinite(v.astype(np.float64)).all() for v in r32.values()), key
        cases.append(key)
        params[key] = meta
        for k, v in dict(r32, **arrays).items():
            if not (key.startswith("l1::") and k in ("a", "b")):          # read from l2::<shape>
                store[f"{key}::{k}"] = v
    for name in HIST:
        key, res, meta = hist_case(ref, name)
        print(f"{key}: {int(np.isfinite(res['scaled']).sum())} pairs")
        cases.append(key)
        params[key] = meta
        for k, v in res.items():
            store[f"{key}::{k}"] = v
    store["meta"] = np.frombuffer(json.dumps({"cases": cases, "params": params}, sort_keys=True).encode(), dtype=np.uint8)
    write_npz(os.path.join(OUT, "g20_pair.npz"), store)
    size = os.path.getsize(os.path.join(OUT, "g20_pair.npz"))
    print("g20_pair.npz", size, "bytes")
    assert size < 1024 * 1024


if __name__ == "__main__":
    main()

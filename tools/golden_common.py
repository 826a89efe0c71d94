"""What the golden generators tools/make_*_golden.py share: where they write, how they load a module of the upstream
reference (from the directory ``oracle/_refshim.py`` points at, at run time only), the byte-reproducible archive writer, the
margin of the reference's own fp32 result against its float64 one, and the contract file."""
import importlib.util
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import _refshim  # noqa: E402

OUT = os.environ.get("GET_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden")


def load_reference(relative_path, module_name):
    path = os.path.join(_refshim.REF, relative_path)
    if not os.path.exists(path):
        raise RuntimeError(f"reference not found at {path}")
    spec = importlib.util.spec_from_file_location(module_name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def to_numpy(res):
    """The result dict of one run with its tensors detached and copied out."""
    return {k: (v.detach().numpy().copy() if torch.is_tensor(v) else v) for k, v in res.items()}


def margin(r32, r64, keys, bound_fn):
    """The reference's fp32 result against its float64 one over `keys`: the worst fraction of a TENTH of the test's bound
    bound_fn(key, float64 result) (an array for an elementwise bound, a number for one on the largest error)."""
    worst = 0.0
    for k in keys:
        want = r64[k].astype(np.float64)
        err = np.abs(r32[k].astype(np.float64) - want)
        worst = max(worst, (err / (0.1 * bound_fn(k, want))).max())
    return worst


def write_npz(path, arrays):
    """np.load-compatible archive with fixed member timestamps, so that a rerun reproduces the file byte for byte."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def write_contract(path, contract):
    with open(path, "w") as fh:
        json.dump(contract, fh, indent=1, sort_keys=True)
        fh.write("\n")

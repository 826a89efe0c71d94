"""The shape of the host layer: get_amd/ops/ is one module per family, the package only re-exports, and
callers look ops up on the package at call time.  Runs without the library."""
import ast
import importlib
import inspect
import os

import pytest

from get_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS_DIR = os.path.join(ROOT, "get_amd", "ops")

# the 61 public names of the package and the module that defines each
PUBLIC = {
    "streams": ["side_stream", "side_join", "pending_side_stream", "side_mark_backward"],
    "weights": ["bump_weight_epoch", "fp32x3p_guard", "transposed", "bf16_twins", "derived", "refresh_transposes"],
    "graph": ["PackedAdj", "graph_build", "as_packed", "RaggedPlan", "spmm", "ggnn_cell", "bf16_cell_ok", "scorer_fusable",
              "fused_dropout_ok", "new_dropout_seed", "dropout_mask_reference", "scorer_gsl", "gsl_topk", "feat_dropout",
              "gat_dropout_mask", "GAT_OUTPUT", "GAT_ELU", "GAT_PLAIN", "gat_layer", "gat_pattern", "gcn_scale", "relu", "GCNAdj"],
    "attention": ["concat_att", "query_att", "tanh_att", "mha_sdpa", "add_layernorm"],
    "rnn": ["lstm_seq", "gru_seq"],
    "bidaf": ["att_flow", "highway"],
    "match": ["soft_align", "LIN_ATT_MODES", "lin_att", "match_dot", "MATCH_BCAST_OPS", "match_bcast", "gauss_kernel"],
    "dense": ["linear", "linear_wgrad_bf16", "Segments", "seg_broadcast", "seg_pad", "evd_assemble", "masked_mean", "cross_entropy",
              "backward", "CLS_EXTRA", "cls_metrics", "adam_step_flat"],
}
FLAGS = ["CLAIM_SIDE_STREAM", "WGRAD_SIDE_STREAM", "WGRAD_FEW_ROWS"]


def test_every_public_name_is_the_object_its_module_defines():
    assert sum(len(v) for v in PUBLIC.values()) == 61
    for mod, names in PUBLIC.items():
        sub = importlib.import_module("get_amd.ops." + mod)
        assert getattr(ops, mod) is sub
        for name in names:
            obj = getattr(ops, name)
            assert obj is getattr(sub, name), name
            if inspect.isfunction(obj) or inspect.isclass(obj):
                assert obj.__module__ == sub.__name__, f"{name} is defined in {obj.__module__}, not in {sub.__name__}"


def test_the_mutable_flags_live_in_streams_only(monkeypatch):
    for name in FLAGS:
        assert hasattr(ops.streams, name) and not hasattr(ops, name), name
        with pytest.raises(AttributeError):
            monkeypatch.setattr(ops, name, False)        # a stale patch must fail, not silently change nothing


def imports_of(path):
    """(level, module, [names]) of every import statement in a file; `import a.b` gives (0, "a.b", [])."""
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom):
            yield node.level, node.module or "", [a.name for a in node.names]
        elif isinstance(node, ast.Import):
            for a in node.names:
                yield 0, a.name, []


def py_files(*dirs):
    for d in dirs:
        for base, _, files in os.walk(os.path.join(ROOT, d)):
            for f in sorted(files):
                if f.endswith(".py"):
                    yield os.path.join(base, f)


def test_no_family_module_imports_the_package():
    submodules = {f[:-3] for f in os.listdir(OPS_DIR) if f.endswith(".py") and f != "__init__.py"}
    assert set(PUBLIC) | {"_util"} == submodules
    for mod in sorted(submodules):
        for level, module, names in imports_of(os.path.join(OPS_DIR, mod + ".py")):
            where = f"get_amd/ops/{mod}.py: level {level} import of {module!r} {names}"
            if level == 0:
                assert module != "get_amd.ops" and not (module == "get_amd" and "ops" in names), where
            elif level == 1 and module == "":
                assert set(names) <= submodules, where       # `from . import streams` names a sibling, never a re-export
            elif level == 2:
                assert module.split(".")[0] != "ops" and "ops" not in names, where


def test_callers_outside_the_package_take_op_functions_from_the_package_at_call_time():
    """tools/bidaf_bench.py and tools/match_bench.py swap ops.att_flow, ops.highway and ops.soft_align by assignment: that
    reaches a caller only while it writes ops.NAME(...).  Classes (PackedAdj) may be imported by name."""
    for path in py_files("get_amd", "tools"):
        if path.startswith(OPS_DIR + os.sep):
            continue
        in_pkg = path.startswith(os.path.join(ROOT, "get_amd") + os.sep)
        for level, module, names in imports_of(path):
            if level == 0 and (module == "get_amd.ops" or module.startswith("get_amd.ops.")):
                target = module
            elif in_pkg and level == 1 and (module == "ops" or module.startswith("ops.")):
                target = "get_amd." + module
            else:
                continue
            owner = importlib.import_module(target)
            for name in names:
                obj = getattr(owner, name)
                assert inspect.isclass(obj), f"{os.path.relpath(path, ROOT)} imports {name} from {target} by name"

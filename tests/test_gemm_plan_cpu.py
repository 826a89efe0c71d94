"""The GEMM planner (csrc/gemm_plan.h: tile choice, fast-path rule, split-K plans, workspace layout, kernel configuration, grid) on
the CPU: tools/gemm_plan_sweep.cpp is built with the host compiler under ASan / UBSan and run as a stand-alone child process.  It
walks the planner over shape classes, checks the invariants the kernels rely on, asserts the plans the project relies on (those
named in tests/test_gpu_gemm_paths.py, the bench step's, and every launch of every case of tests/test_gpu_cell_paths.py: tile,
split with chunk count and finish shape, fast or generic, workspace or atomic, column sums fused or separate) exactly, and exits
non-zero on any violation."""
import pathlib
import re
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
CLANG = pathlib.Path("/opt/rocm/llvm/bin/clang++")


def test_planner_is_host_code_that_only_the_batch_file_includes():
    """gemm_plan.h and gemm_types.h include nothing of HIP, and in csrc/ only gemm_batch.hip includes gemm_plan.h -- the Makefile
    relies on it (an edit of a plan rebuilds that one object, not the kernels)."""
    csrc = ROOT / "get_amd" / "csrc"
    for name in ("gemm_plan.h", "gemm_types.h"):
        incs = re.findall(r'^\s*#\s*include\s+[<"]([^>"]+)[>"]', (csrc / name).read_text(), re.M)
        assert incs and all(i in ("gemm_types.h", "stdint.h", "stddef.h", "string.h") for i in incs), (name, incs)
    users = [p.name for p in sorted(list(csrc.glob("*.hip")) + list(csrc.glob("*.h")))
             if re.search(r'^\s*#\s*include\s+"gemm_plan\.h"', p.read_text(), re.M)]
    assert users == ["gemm_batch.hip"]
    engine = [p.name for p in sorted(list(csrc.glob("*.hip")) + list(csrc.glob("*.h")))
              if re.search(r'^\s*#\s*include\s+"gemm_engine\.h"', p.read_text(), re.M)]
    assert engine == ["gemm_batch.hip", "gemm_ops.hip"]


@pytest.mark.skipif(not CLANG.is_file(), reason="no host compiler at /opt/rocm/llvm/bin/clang++")
def test_gemm_plan_sweep(tmp_path):
    exe = tmp_path / "gemm_plan_sweep"
    subprocess.run([str(CLANG), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tools" / "gemm_plan_sweep.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)      # a stand-alone binary
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:]
    assert "no violation" in run.stdout and "VIOLATION" not in run.stdout.replace("no violation", "")

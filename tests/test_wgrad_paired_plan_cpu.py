"""Which weight-gradient products take the paired-column GEMM: the plan rule on the CPU.

``make paired-plan-check`` compiles tests/host/gemm_paired_plan_check.cpp -- a stand-alone
program of layer_plans.h's plan functions, built with ``-fsanitize=address,undefined`` --
and runs it: the qualifying shapes (the bench's 256 x 256 layer in 128 slabs, 512-wide
layers, one tile in one slab, a ragged last slab, leading dimensions beyond the widths,
slab rows just inside 2^31 bytes), the switch off, and one refused product per condition
of the rule (orientation, gathers, epilogue, accumulation, H / bias / head, sides that
are no multiple of 128, a column-major or odd-strided or 4-B-aligned C, an odd slab
stride, operands that are not 16-B vectors, leading dimensions or slab extents beyond
32-bit byte offsets), and the plan's earlier arms keeping their products.  Tile, grid,
threads, ``k_per_split`` and the profiling kind are the one kernel's either way.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_paired_column_plan_rule():
    out = subprocess.run(['make', '-C', ROOT, 'paired-plan-check'], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert 'paired plan ok' in out.stdout


def test_switch_is_declared_to_python():
    from garage_amd import _lib
    assert _lib.load().ga_set_wgrad_paired_columns(1) == 0

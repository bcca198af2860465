"""CPU checks of the boundary: the library loads and exports exactly the symbols
the header declares; the ctypes structs match the header's layout; the product
never imports the oracle."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    text = open(os.path.join(ROOT, 'include', 'garage_amd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(ga_[a-z0-9_]+)\s*\(', text)))


def _dynamic_symbols(path):
    """(type, name) of every defined dynamic symbol of the shared library."""
    nm = shutil.which('nm') or '/opt/rocm/llvm/bin/llvm-nm'
    out = subprocess.run([nm, '-D', '--defined-only', path], capture_output=True,
                         text=True, check=True).stdout
    return [tuple(line.split()[-2:]) for line in out.splitlines() if line.strip()]


def test_library_exports_every_declared_symbol():
    """... and nothing else: every other function is hidden (-fvisibility=hidden,
    GA_API on the header's declarations), so a definition that drifts from its
    declaration fails to compile instead of exporting a second symbol."""
    from garage_amd import _lib
    lib = _lib.load()
    names = _header_symbols()
    assert len(names) >= 20
    for name in names:
        assert hasattr(lib, name), name
    # the ctypes table and the header must describe the same set
    assert sorted(_lib.SIGNATURES) == names
    assert lib.ga_abi_version() == 5
    syms = _dynamic_symbols(_lib.LIB_PATH)
    functions = sorted(n for t, n in syms if t in ('T', 'W'))
    assert functions == names
    assert not [n for _, n in syms if n.startswith('_Z')]
    data = [n for t, n in syms if t not in ('T', 'W')]
    assert data and all(n.startswith('__hip_cuid_') for n in data), data


def test_ctypes_structs_match_the_header():
    """sizeof / offsetof / field sizes of the header's structs, from a C program
    compiled by the host compiler, against the ctypes mirrors in _lib.py."""
    from garage_amd import _lib
    structs = {'ga_mlp_desc': _lib.MlpDesc, 'ga_synth_env': _lib.SynthEnv,
               'ga_head_args': _lib.HeadArgs, 'ga_record_args': _lib.RecordArgs,
               'ga_norm_args': _lib.NormArgs, 'ga_update_args': _lib.UpdateArgs}
    lines = ['#include <stddef.h>', '#include <stdio.h>',
             '#include "garage_amd.h"', 'int main(void) {']
    want = []
    for cname, py in structs.items():
        lines.append('printf("{0} %zu\\n", sizeof({0}));'.format(cname))
        want.append('{} {}'.format(cname, ctypes.sizeof(py)))
        for field, ftype in py._fields_:
            lines.append('printf("{0}.{1} %zu %zu\\n", offsetof({0}, {1}), '
                         'sizeof((({0}*)0)->{1}));'.format(cname, field))
            want.append('{}.{} {} {}'.format(cname, field,
                                             getattr(py, field).offset,
                                             ctypes.sizeof(ftype)))
    lines += ['return 0;', '}']
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, 'layout.c'), os.path.join(tmp, 'layout')
        with open(src, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        subprocess.run(['cc', '-std=c99', '-Wall', '-Werror', '-I',
                        os.path.join(ROOT, 'include'), src, '-o', exe], check=True)
        got = subprocess.run([exe], capture_output=True, text=True,
                             check=True).stdout.split('\n')[:-1]
    assert got == want


def test_argument_errors_are_reported_without_a_gpu():
    from garage_amd import _lib
    with pytest.raises(_lib.GarageAmdError) as e:
        _lib.call('ga_gae_scan_f32', None, None, None, None, None, 1, 1, 1, 1,
                  0, 1, 0.99, 0.97, 0.0, 0.0, None, None, None)
    assert 'null pointer' in str(e.value)


def test_product_never_imports_the_oracle():
    bad = []
    for base, _, files in os.walk(os.path.join(ROOT, 'garage_amd')):
        for f in files:
            if f.endswith(('.py', '.hip', '.cpp', '.h')):
                src = open(os.path.join(base, f)).read()
                if re.search(r'^\s*(from|import)\s+oracle\b', src, flags=re.M):
                    bad.append(f)
    assert not bad, bad


def test_host_loops_under_address_sanitizer():
    """``make asan-host``: the C++ epoch loops (update.cpp) compiled with ``-fsanitize=address,undefined`` for the CPU
    and run against recording fakes of every kernel entry point
    (tests/host/update_loop_harness.cpp, suite loops): minibatch ranges, the data-parallel even
    split and per-step scales, phase 1, the interleaving of two passes, argument
    errors, the fused step's scratch layout and regions (the rollout loop has its own
    harness, ``make asan-env-loop``).  GPU sanitizers are not available on this pool."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run(['make', '-C', root, 'asan-host'], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert 'host loops ok' in out.stdout


def test_mlp_layer_dispatch_under_address_sanitizer():
    """``make asan-mlp``: the per-layer MLP dispatch (mlp_layers.cpp) compiled with
    ``-fsanitize=address,undefined`` for the CPU, with the library's own kernel-choice
    rules (layer_plans.h), and run against recording fakes of the launch seam below
    them (tests/host/mlp_layers_harness.cpp).  Each fake checks the extent its kernel
    would reach against the exactly-sized buffer the pointer came from -- ragged
    widths, LayerNorm offsets, slabs x splits, the head layer's transposed weight
    gradient, the weight planes -- and that the plan's grid covers the product; which
    launcher a layer takes under every switch and at shapes a kernel refuses; that the
    pair launch's weight-gradient descriptors are the single launch's; and the plans
    against literal tables with both sides of every boundary."""
    out = subprocess.run(['make', '-C', ROOT, 'asan-mlp'], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert 'mlp layers ok' in out.stdout


def test_driver_build_entry_point():
    """``__graft_entry__.build()`` -- what the driver runs on a CPU-only machine --
    compiles (a no-op when the library is current), imports the package and agrees
    with the loader on the ABI version."""
    import __graft_entry__ as entry
    from garage_amd import _lib
    entry.build()
    assert _lib.load().ga_abi_version() == _lib.ABI_VERSION

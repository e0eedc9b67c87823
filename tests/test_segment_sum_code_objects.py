"""CPU: the segmented row sum (csrc/segment_sum_rows.hip), read through scripts/kernel_resources.py, uses no scratch memory
and spills no register, and its object holds that kernel family only (one instantiation per 16-bit dtype): a pure stream must
not cost more than the bytes it moves."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import kernel_resources as KR  # noqa: E402

KERNELS = [('segment_sum_rows.o', 'segment_sum_rows_kernel<BF16>'), ('segment_sum_rows.o', 'segment_sum_rows_kernel<F16>')]


@pytest.fixture(scope='module')
def table():
    if not KR.tools_available():
        pytest.skip('llvm-objcopy / clang-offload-bundler / llvm-readelf not found under /opt/rocm')
    import __graft_entry__  # noqa: F401  (puts the package on sys.path)
    import importlib.util
    spec = importlib.util.spec_from_file_location('bp_build_hip', os.path.join(ROOT, 'backpacks-flash-attn_amd', 'build_hip.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()   # no-op when the objects are current
    ks = KR.kernels([os.path.join(KR.BUILD, o) for o in sorted({o for o, _ in KERNELS})])
    return {(k['object'], k['name']): k for k in ks}


@pytest.mark.parametrize('obj,name', KERNELS, ids=[k[1] for k in KERNELS])
def test_segment_sum_kernel_has_no_scratch_and_no_spills(table, obj, name):
    k = table.get((obj, name))
    assert k is not None, 'kernel not found in %s: %s (have %s)' % (obj, name, sorted(n for o, n in table if o == obj))
    assert k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, k
    assert k['private_segment_fixed_size'] == 0, k
    # 8 rows of 16 bytes in flight and 8 fp32 sums per thread: nowhere near the registers of one wave per SIMD
    assert k['vgpr_count'] <= 128, k


def test_the_object_holds_no_other_kernel(table):
    assert sorted(table) == sorted(KERNELS)

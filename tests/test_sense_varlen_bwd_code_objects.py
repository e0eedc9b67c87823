"""CPU: the code objects of the packed sense-mix backward (sense_mix_bwd_varlen.o, sense_dp_slab_varlen.o) through
scripts/kernel_resources.py, as tests/test_code_objects.py does for the fixed-length ones: the instantiations a Backpack-Small
training step launches (d_k = 48, 768 columns) use no scratch and spill nothing, and every instantiation's static LDS stays
inside the budget its kernel declares."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import kernel_resources as KR  # noqa: E402

# (object, kernel, waves per SIMD the registers must still allow)
HOT = [
    ('sense_mix_bwd_varlen.o', 'sense_mix_dc_kernel<Varlen<BF16>, 3, true>', 2),
    ('sense_mix_bwd_varlen.o', 'sense_mix_dc_kernel<Varlen<F16>, 3, true>', 2),
    ('sense_mix_bwd_varlen.o', 'sense_dq_kernel<Varlen<BF16>, 3>', 3),
    ('sense_mix_bwd_varlen.o', 'sense_dk_kernel<Varlen<BF16>, 3>', 3),
    ('sense_dp_slab_varlen.o', 'sense_dp_slab_varlen_kernel<BF16>', 4),
    ('sense_dp_slab_varlen.o', 'sense_dp_slab_varlen_kernel<F16>', 4),
]
# static LDS: the ring kernels one workgroup per CU (160 KB), the slab product two (DpSlabCfg's static_assert: 64 KB)
LDS_BUDGET = {'sense_mix_dc_kernel': 160 * 1024, 'sense_dq_kernel': 160 * 1024, 'sense_dk_kernel': 160 * 1024,
              'sense_dp_slab_varlen_kernel': 64 * 1024}


@pytest.fixture(scope='module')
def table():
    if not KR.tools_available():
        pytest.skip('llvm-objcopy / clang-offload-bundler / llvm-readelf not found under /opt/rocm')
    import __graft_entry__
    __graft_entry__.build()   # no-op when the objects are current
    ks = KR.kernels([os.path.join(KR.BUILD, o) for o in sorted({e[0] for e in HOT})])
    return {(k['object'], k['name']): k for k in ks}


@pytest.mark.parametrize('entry', HOT, ids=[e[1] for e in HOT])
def test_hot_packed_backward_kernel_has_no_scratch(table, entry):
    obj, name, min_waves = entry
    k = table.get((obj, name))
    assert k is not None, 'kernel not found in %s: %s' % (obj, name)
    assert k['vgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0, k
    assert k['waves_per_simd'] >= min_waves, k


def test_every_instantiation_stays_inside_its_lds_budget(table):
    assert len(table) == 2 * (16 + 8 + 8) + 2        # dC: KD x FULL, dq and dk: KD, per dtype; the slab product per dtype
    for (obj, name), k in table.items():
        assert k['group_segment_fixed_size'] <= LDS_BUDGET[name.split('<')[0]], k

"""CPU: register account of the inference-only add + LayerNorm instantiations (csrc/add_layer_norm.hip,
add_layer_norm_chain_kernel behind bp_add_layer_norm_chain) at the trunk width of Backpack-Small, cols = 768 = three chunks per lane: the third
input stream, the table addresses and the raw words of a whole row in flight must fit the registers -- no scratch, no
spills, eight waves per SIMD.  Read through scripts/kernel_resources.py like tests/test_code_objects.py."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import kernel_resources as KR  # noqa: E402

# add_layer_norm_chain_kernel<ET, CH, W_F32, EMB, X0B, X1, XOUT>: the launches of the chained trunk forward
FORMS = {'ln_0 (embedding, z alone)': 'true, false, false, false',
         'first norm1 (embedding + branch)': 'true, true, false, true',
         'norm2 (peek: z alone)': 'false, false, true, false',
         'later norm1 (settle: three inputs, residual out)': 'false, true, true, true'}
CASES = [('add_layer_norm_chain_kernel<%s, 3, %s, %s>' % (et, w, flags), what)
         for et in ('BF16', 'F16') for w in ('false', 'true') for what, flags in FORMS.items()]


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
    return {k['name']: k for k in KR.kernels([os.path.join(KR.BUILD, 'add_layer_norm.o')])}


@pytest.mark.parametrize('name, what', CASES, ids=[c[0] for c in CASES])
def test_chain_instantiation_uses_no_scratch(table, name, what):
    k = table.get(name)
    assert k is not None, 'kernel not found in add_layer_norm.o: %s (%s)' % (name, what)
    assert k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, k
    assert k['private_segment_fixed_size'] == 0, k
    assert k['waves_per_simd'] == 8, k


def test_todays_instantiations_are_still_there(table):
    # <ET, CH, RES_F32, W_F32, NTL, NTS, NTZ, SCALED>: untouched by the inference forms, which are a kernel of their own
    for et in ('BF16', 'F16'):
        for scaled in ('false', 'true'):
            name = 'add_layer_norm_kernel<%s, 3, true, true, true, true, false, %s>' % (et, scaled)
            assert name in table and table[name]['private_segment_fixed_size'] == 0, name

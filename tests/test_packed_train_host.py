"""CPU: training on packed batches -- packed_lm_labels against a loop, the default config's refusal, the three new entry points
in the header, the ctypes table and the library (ABI still 11: additive)."""
import pytest
import torch

import bp_hip
from decode_support import _nano_backpack
from src.utils.packing import pack_sequences, packed_lm_labels
from test_abi import declared_prototypes

BACKWARD = ('bp_sense_mix_dc_varlen', 'bp_sense_dp_slab_varlen', 'bp_sense_dq_dk_varlen')


@pytest.mark.parametrize('seqs', [[[5, 6, 7], [8], [], [9, 10, 11, 12]], [[], [], [3, 4]], [[1], [2], [3]], [[1, 2, 3, 4]]])
def test_packed_lm_labels_against_a_loop(seqs):
    ids, cu, _ = pack_sequences(seqs)
    want = [tok for s in seqs for tok in (list(s[1:]) + [-100] if s else [])]
    assert packed_lm_labels(ids, cu).tolist() == want
    assert packed_lm_labels(ids, cu, ignore_index=-1).tolist() == [-1 if t == -100 else t for t in want]
    assert ids.tolist() == [t for s in seqs for t in s]                      # the ids themselves are left alone


def test_the_default_config_still_refuses_gradients():
    nano = _nano_backpack(seed=3)
    assert nano.config.packed_train is False and nano.transformer.packed_train is False
    packed, cu, longest = pack_sequences([[1, 2, 3], [4, 5]])
    with pytest.raises(RuntimeError, match='inference-only'):
        nano(packed, cu_seqlens=cu, max_seqlen=longest)


def test_header_table_and_library_agree_on_the_backward_entries():
    protos, handle = declared_prototypes(), bp_hip.lib()
    for name in BACKWARD:
        assert name in protos and name in bp_hip.SIGNATURES and hasattr(handle, name), name
        assert protos[name][0] == 'int' and len(protos[name][1]) == len(bp_hip.SIGNATURES[name][1])
    assert bp_hip.ABI_VERSION == 11 and handle.bp_abi_version() == 11

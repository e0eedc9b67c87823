"""CPU: the shipped table of pinned hipBLASLt solutions (backpacks-flash-attn_amd/bp_hip/gemm_solutions.json) parses, every
entry states the spread it had to beat and the library version it was measured with, and no row applies below 131 072
rows -- so decoding, the generation goldens and every small-shape test keep torch's GEMMs."""
import json

import bp_hip
from bp_hip import gemm


def _spec():
    with open(gemm.TABLE_PATH) as f:
        return json.load(f)


def test_shipped_table_parses():
    spec = _spec()
    table = bp_hip.GemmTable(spec)
    assert isinstance(spec['library_version'], int) and spec['library_version'] > 0 and spec['arch']
    pinned = [e for e in spec['entries'] if e.get('solution') is not None]
    assert table.n_rows == len(pinned)
    for i, e in enumerate(pinned):
        row = table.rows[i]
        assert (row.n, row.k, row.m_min, row.solution) == (e['n'], e['k'], e['m_min'], e['solution'])
        assert row.arch.decode() == e.get('arch', spec['arch']) and row.version == e.get('library_version', spec['library_version'])
    for m, rows in table.chunk_rows.items():
        assert m >= gemm.M_BUCKET_MIN and (rows == 0 or (rows >= gemm.M_BUCKET_MIN and m % rows == 0))


def test_every_entry_names_its_spread_and_library_version():
    for e in _spec()['entries']:
        assert e['dtype'] in gemm.DTYPES and e['epilogue'] in gemm.EPILOGUES, e
        assert isinstance(e['library_version'], int) and e['library_version'] > 0 and e['arch'], e
        assert e['spread_ms'] >= 0 and e['heuristic_ms'] > 0 and e['n_per_candidate'] >= 10, e
        if e.get('solution') is not None:
            # admitted only because it beat the heuristic's first pick by more than that pick's spread
            assert e['solution'] >= 0 and e['heuristic_ms'] - e['pinned_ms'] > e['spread_ms'], e


def test_no_entry_applies_below_the_m_bucket():
    assert gemm.M_BUCKET_MIN == 131072
    for e in _spec()['entries']:
        assert e['m_min'] >= gemm.M_BUCKET_MIN, e
    table = gemm.shipped_table()
    assert all(floor >= gemm.M_BUCKET_MIN for floor in table.floor.values())


def test_linear_is_torch_without_a_device():
    import torch
    x, w, b = torch.randn(5, 3, 8), torch.randn(4, 8), torch.randn(4)
    assert torch.equal(bp_hip.linear(x, w, b), torch.nn.functional.linear(x, w, b))
    out = torch.empty(15, 4)
    bp_hip.linear(x, w, out=out)
    assert torch.equal(out, x.reshape(15, 8) @ w.t())

"""The batches of sst_encode_cases.py reach the edges they claim, for every
tile size the gather kernel may report; and the module's expected bytes are
the committed reference-layout fixtures' for the golden table.  No GPU."""
import base64
import json
import os

import numpy as np
import pytest

import sst_encode_cases as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("T", S.TILES)
def test_tile_edges_meet_every_record_byte_and_a_table_start(T):
    b = S.tile_records(T)
    assert b.sorted_tables()
    ph = S.edge_phases(b, T)
    for q in range(S.HDR):
        assert q in ph, f"no tile edge in header byte {q}"
    assert S.HDR + S.EDGE_KLEN in ph, "no tile edge at a key/value boundary"
    assert 0 in ph, "no tile edge at a record boundary"
    assert any(o % T == 0 for o in S.table_starts(b)), "no tile edge at a table boundary"


@pytest.mark.parametrize("T", S.TILES)
@pytest.mark.parametrize("plus", [0, 1])
def test_tile_sized_arenas(T, plus):
    b = S.tile_sized(T, 3, plus)
    assert b.rec_off()[1] == 3 * T + plus and b.ntab == 3 and (np.diff(b.first.astype(np.int64)) > 0).all()


def test_lengths_and_residues_are_all_there():
    b = S.lengths_alignment()
    assert b.sorted_tables()
    c = b.ents
    assert set(c["klen"].tolist()) == set(range(49)) == set(c["vlen"].tolist())
    for kl in range(1, 49):
        assert set((c["key_off"][c["klen"] == kl] % 16).tolist()) == set(range(16))
        assert set((c["val_off"][c["vlen"] == kl] % 16).tolist()) == set(range(16))
    for base in (0, 1, 3, 15):
        kp, vp = S.residue_pairs(b, base)
        assert len(kp) == 256 and len(vp) == 256  # every (source, destination) residue pair
    # an empty key is only ever a table's first
    empty = np.nonzero(c["klen"] == 0)[0]
    assert len(empty) > 16 and set(empty.tolist()) <= set(b.first[:-1].tolist())


def test_small_and_step_batches():
    assert [len(b.expected()[0]) for b in S.smallest()] == [8, 9, 9, 10]
    e = S.empty_tables(5).expected()
    assert len(e[0]) == 0 and e[1].tobytes() == b"\0" * 40 and e[2]["index_len"].tolist() == [8] * 5
    p = S.empty_table_places()
    assert np.diff(p.first.astype(np.int64)).tolist() == [0, 3, 0, 0, 150, 2, 0] and p.sorted_tables()
    assert S.two_in_a_chunk().expected()[0].tobytes() == b"\0" * 16
    s = S.index_steps()
    assert s.sorted_tables() and np.diff(s.first.astype(np.int64)).tolist() == list(S.STEP_SIZES)
    data, index, spans, _, _ = s.expected()
    counts = [int.from_bytes(index[int(o):int(o) + 8].tobytes(), "little") for o in spans["index_off"]]
    assert counts == list(S.STEP_COUNTS)
    assert 0 in s.ents["klen"][s.first[:-1].astype(np.int64)] and s.ents["klen"].max() == 40
    for b in (s, p, S.lengths_alignment(), S.shared_arena(), S.one_value()):
        assert b.sizes_only() == (len(b.expected()[0]), len(b.expected()[1])), b


def test_other_batches_are_sorted_and_invalid_ones_are_not():
    for b in (S.shared_arena(), S.one_value(), S.ok_across_boundary(), S.tile_sized(256, 3, 1)):
        assert b.sorted_tables(), b
    sh = S.shared_arena()
    assert sh.vals is sh.keys and sh.ntab > 10
    z = S.zipf_tables(n=20_000)
    assert z.sorted_tables() and z.ntab > 10
    sizes = z.expected()[2]["data_len"]
    assert sizes.min() < 8192 and sizes.max() > 500_000
    for name, args, idx, alone in S.invalid_cases():
        b = S.Batch(name, *args)
        if name in ("equal_keys", "prefix_after", "decreasing", "first_of_several", "second_table"):
            assert not b.sorted_tables(), name
    keys, ents, first = S.big_entries()
    b = S.Batch("big", keys, np.zeros(0, np.uint8), ents, first)
    assert b.rec_off()[1] > 1 << 32 and len(ents) == 1070
    assert int(b.rec_off()[0][int(first[2])]) > 1 << 32  # a table that starts past 4 GiB


def test_expected_bytes_are_the_golden_tables():
    """keys str(i), values str(i*100), i < 500, in bytewise order: the committed fixtures."""
    ents = sorted((str(i).encode(), str(i * 100).encode()) for i in range(500))
    data, index = S.table_files(ents)
    assert data == open(os.path.join(GOLDEN, "sstable_test_data.db"), "rb").read()
    assert index == open(os.path.join(GOLDEN, "sstable_test_index.db"), "rb").read()
    klen = np.array([len(k) for k, _ in ents])
    vlen = np.array([len(v) for _, v in ents])
    b = S.Batch("golden", np.frombuffer(b"".join(k for k, _ in ents), np.uint8),
                np.frombuffer(b"".join(v for _, v in ents), np.uint8),
                S.entries(np.cumsum(klen) - klen, klen, np.cumsum(vlen) - vlen, vlen), [0, 500])
    d, x, spans, dsha, isha = b.expected()
    assert d.tobytes() == data and x.tobytes() == index and spans[0].tolist() == (0, len(data), 0, len(index))
    js = json.load(open(os.path.join(GOLDEN, "sstable_test_checksum.db")))
    assert base64.b64encode(dsha[0].tobytes()).decode() == js["data_checksum"]
    assert base64.b64encode(isha[0].tobytes()).decode() == js["index_checksum"]

"""Positions out of searchlite's posting file (slf_postings_decode_positions, index_files.decode_positions,
load_index(positions=True)): the restated writer (oracle/segfile_writer.py: a count per posting, then the deltas
of its positions) read back through the new decode call, beside the arrays slf_postings_decode gives."""
import numpy as np

from oracle import segfile_writer as SW
from searchlite_amd import index_files as IF
from searchlite_amd.segment import SegmentBuilder


def image(terms, keep_positions=True):
    """terms: [(doc ids, tfs, positions per posting or None)] -> (file image, offsets)"""
    blob, offs = bytearray(), []
    for d, t, p in terms:
        offs.append(len(blob))
        blob += SW.write_term(d, t, p, keep_positions)
    return bytes(blob), np.array(offs, np.uint64)


def test_explicit_positions_roundtrip():
    """postings with several, one and no positions; 200 postings (block-max arrays in front of them); deltas of
    more than one varint byte"""
    many = [[i, i + 1, i + 300, i + 70000] for i in range(200)]
    terms = [([1, 5, 9], [2, 1, 3], [[0, 7], [], [4, 4, 1000000]]),
             (list(range(0, 400, 2)), [4] * 200, many),
             ([3], [1], [[2 ** 31 - 1]]),
             ([], [], [])]
    post, offs = image(terms)
    dec = IF.decode_postings(post, offs)
    po, ps = IF.decode_positions(post, offs)
    assert dec["doc_ids"].tolist() == [1, 5, 9] + list(range(0, 400, 2)) + [3]
    assert len(po) == len(dec["doc_ids"]) + 1 and po.dtype == np.uint64 and ps.dtype == np.uint32
    want = [p for _, _, plist in terms for p in plist]
    got = [ps[int(po[i]):int(po[i + 1])].tolist() for i in range(len(po) - 1)]
    assert got == want and int(po[-1]) == len(ps) == 2 + 0 + 3 + 800 + 1


def test_a_file_written_without_positions_gives_empty_lists():
    post, offs = image([([1, 5, 9], [2, 1, 3], None), ([2], [1], None)], keep_positions=False)
    po, ps = IF.decode_positions(post, offs)
    assert po.tolist() == [0, 0, 0, 0, 0] and len(ps) == 0
    # keep_positions with no positions recorded: a zero count per posting
    post, offs = image([([1, 5], [2, 1], None)])
    po, ps = IF.decode_positions(post, offs)
    assert po.tolist() == [0, 0, 0] and len(ps) == 0


def test_too_small_a_positions_array_and_a_truncated_file():
    import ctypes as C
    post, offs = image([([1, 5], [2, 1], [[0, 7], [3]])])
    L = IF._load()
    img = np.frombuffer(post, np.uint8)
    po, ps, total = np.zeros(3, np.uint64), np.zeros(2, np.uint32), C.c_uint64(0)
    assert L.slf_postings_decode_positions(img.ctypes.data, len(img), offs.ctypes.data, 1, None, None, 0, C.addressof(total)) == 0
    assert total.value == 3
    assert L.slf_postings_decode_positions(img.ctypes.data, len(img), offs.ctypes.data, 1, po.ctypes.data, ps.ctypes.data, 2, None) < 0
    assert b"positions_cap" in L.slf_last_error()
    assert L.slf_postings_decode_positions(img.ctypes.data, len(img) - 1, offs.ctypes.data, 1, None, None, 0, None) < 0


def test_write_index_with_positions_through_load_index(tmp_path):
    sb = SegmentBuilder(["body"])
    sb.add_document("a", {"body": "olive oil and olive pasta"})
    sb.add_document("b", {"body": "oil oil oil"})
    seg = sb.build()
    with_pos, without = str(tmp_path / "with"), str(tmp_path / "without")
    SW.write_index(with_pos, [seg], keep_positions=True)
    SW.write_index(without, [seg], keep_positions=False)
    plain = IF.load_index(with_pos).segments[0]
    assert plain.pos_offsets is None and plain.positions is None  # the switch is off by default
    got = IF.load_index(with_pos, positions=True).segments[0]
    assert np.array_equal(got.doc_ids, seg.doc_ids) and np.array_equal(got.tfs, seg.tfs)
    # write_index records positions 0 .. tf - 1 for every posting
    assert got.pos_offsets.tolist() == np.concatenate([[0], np.cumsum(seg.tfs)]).tolist()
    assert got.positions.tolist() == [p for tf in seg.tfs for p in range(int(tf))]
    assert got.posting_positions(got.term_id("body:oil"), 1).tolist() == [0, 1, 2]
    bare = IF.load_index(without, positions=True).segments[0]
    assert bare.pos_offsets.tolist() == [0] * (seg.n_postings + 1) and len(bare.positions) == 0

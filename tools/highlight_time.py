"""Time of the highlighter (slg_highlight_batch) at config 2's shape: 1024 queries x their top-10 hits, one field
spec of 3 terms per query, fragment_size 160, over texts of about 1 KB and about 8 KB (word soup over the generated
vocabulary of tools/vocabulary.py, Zipf-like word choice), number_of_fragments 1 and 5.  Per shape, mean of `reps`
calls after two warm-up calls, `rounds` times over so the spread shows:
  * slg_highlight_batch with arrays sized beforehand: the whole call by the host clock (the call ends in a stream
    synchronise), and its own split into the count part (uploads, count + scan kernels, the totals back, the wait)
    and the emit part (emit kernel, the strings back, the wait) (slg_highlight_phase_ms);
  * the text bytes the count pass has to scan — per item up to the end of its last match, or the whole text if it has
    fewer than number_of_fragments matches, computed here from the answer — as bytes/s of the whole call and of the
    count part against the 8.0 TB/s HBM peak.  These are whole-call rates, not a kernel's share of peak: kernel times
    come from `rocprofv3 --kernel-trace --stats -- python tools/highlight_time.py 3 1`, in a run of its own;
  * the same items through the host TU's sequential highlighter (csrc/slg_highlight_capi.cpp, slgx_hl_reference) on
    this box, on 16 threads.
The device's answer is compared with the host highlighter's, byte for byte, before anything is timed.
usage (GPU box): python tools/highlight_time.py [reps] [rounds]"""
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from searchlite_amd import build, searcher, _native as N  # noqa: E402
from searchlite_amd.highlight import highlight_spec, pack_specs  # noqa: E402
from searchlite_amd.segment import Segment  # noqa: E402
from tools.vocabulary import make_vocabulary  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
nq, k, n_docs, vocab = 1024, 10, 8000, 1 << 14
HBM_PEAK = 8.0e12

L = C.CDLL(build.build_plan_lib())
err = C.create_string_buffer(512)


def texts_of(rng, words, mean_bytes):
    """n_docs texts of about mean_bytes: words by a Zipf-like rank, separated by a blank, a sentence end now and then"""
    out, at = [], 0
    for d in range(n_docs):
        target = int(mean_bytes * (0.5 + rng.random()))
        ranks = np.minimum((rng.pareto(1.1, size=target // 3 + 2) * 8).astype(np.int64), vocab - 1)
        parts, n = [], 0
        for r in ranks:
            if n >= target:
                break
            at += 1
            parts.append(words[int(r)].capitalize() + "." if at % 11 == 0 else words[int(r)])
            n += len(parts[-1]) + 1
        out.append(" ".join(parts).encode())
    return out


def dummy_segment():
    return Segment(n_docs=n_docs, term_offsets=np.array([0, 1], np.uint64), doc_ids=np.zeros(1, np.uint32),
                   tfs=np.ones(1, np.uint32), field_doc_len=[np.ones(n_docs, np.float32)], field_avgdl=np.ones(1, np.float32),
                   docs=float(n_docs))


def arrays(n_items, n_frags, n_bytes):
    st, io = np.zeros(max(n_items, 1), np.uint8), np.zeros(n_items + 1, np.uint32)
    to, tx = np.zeros(n_frags + 1, np.uint32), np.zeros(max(n_bytes, 1), np.uint8)
    out = N.HlOut(C.sizeof(N.HlOut), n_items, n_frags, n_bytes, st.ctypes.data, io.ctypes.data, to.ctypes.data, tx.ctypes.data, 0, 0, 0)
    return out, (st, io, to, tx)


words = make_vocabulary(vocab)
rng = np.random.default_rng(5)
for mean_bytes in (1024, 8192):
    t0 = time.time()
    texts = texts_of(rng, words, mean_bytes)
    ix = searcher.GpuIndex([dummy_segment()])
    ix.set_stream(torch.cuda.current_stream().cuda_stream)
    field = ix.add_text_field([texts])
    hit_doc = rng.integers(0, n_docs, size=nq * k).astype(np.uint32)
    hit_seg = np.zeros(nq * k, np.uint32)
    hoffs = (np.arange(nq + 1) * k).astype(np.uint32)
    # 3 terms per query: one frequent, one of the middle ranks, one rare word
    q_terms = [[words[int(rng.integers(0, 50))], words[int(rng.integers(50, 2000))], words[int(rng.integers(2000, vocab))]]
               for _ in range(nq)]
    print(json.dumps(dict(texts=n_docs, mean_text_bytes=int(np.mean([len(t) for t in texts])), queries=nq, hits_per_query=k,
                          setup_s=round(time.time() - t0, 1))), flush=True)
    for nf in (1, 5):
        specs = [[highlight_spec(field, q_terms[q], fragment_size=160, number_of_fragments=nf)] for q in range(nq)]
        soffs, arr, keep = pack_specs(specs)
        size = N.HlOut(struct_size=C.sizeof(N.HlOut))

        def call(out):
            N.check(ix._lib.slg_highlight_batch(ix._h, nq, hoffs.ctypes.data, hit_seg.ctypes.data, hit_doc.ctypes.data,
                                                soffs.ctypes.data, arr, C.addressof(out)))
        call(size)
        out, (st, io, to, tx) = arrays(int(size.n_items), int(size.n_frags), int(size.text_bytes))
        call(out)
        # the host highlighter on the same items: the texts of the hits back to back, item i under spec i // k
        item_texts = [texts[int(d)] for d in hit_doc]
        toffs = np.zeros(len(item_texts) + 1, np.uint64)
        np.cumsum([len(t) for t in item_texts], out=toffs[1:])
        blob = np.frombuffer(b"".join(item_texts) + b"\0", np.uint8)
        item_spec = (np.arange(nq * k) // k).astype(np.uint32)
        hout, (hst, hio, hto, htx) = arrays(int(size.n_items), int(size.n_frags), int(size.text_bytes))

        def host_loop(n_threads):
            t = time.perf_counter()
            rc = L.slgx_hl_reference(C.c_uint32(nq * k), C.c_void_p(toffs.ctypes.data), C.c_void_p(blob.ctypes.data),
                                     C.c_void_p(item_spec.ctypes.data), C.c_uint32(nq), arr, C.c_uint32(n_threads),
                                     C.c_void_p(C.addressof(hout)), err, C.c_uint32(512))
            ms = (time.perf_counter() - t) * 1e3
            assert rc == 0, err.value
            return ms
        host_loop(16)
        assert st.tolist() == hst.tolist() and io.tolist() == hio.tolist() and to.tolist() == hto.tolist()   # the same answer
        assert tx.tobytes() == htx.tobytes()
        # what the count pass has to read: up to the end of the item's last match, or all of it
        scanned = 0
        for i, t in enumerate(item_texts):
            n = int(io[i + 1]) - int(io[i])
            if n < nf:
                scanned += len(t)
                continue
            rx = re.compile(b"|".join(rb"\b" + re.escape(w.encode()) + rb"\b" for w in q_terms[i // k]), re.A | re.I)
            at = 0
            for _ in range(nf):
                at = rx.search(t, at).end()
            scanned += at
        call(out)
        for rnd in range(rounds):
            whole, cnt, emit = [], [], []
            for _ in range(reps):
                t = time.perf_counter()
                call(out)
                whole.append((time.perf_counter() - t) * 1e3)
                c, e = ix.highlight_phase_ms()
                cnt.append(c)
                emit.append(e)
            cpu16 = min(host_loop(16) for _ in range(3))
            call_ms, count_ms = float(np.mean(whole)), float(np.mean(cnt))
            print(json.dumps(dict(mean_text_bytes=mean_bytes, number_of_fragments=nf, round=rnd, items=int(size.n_items),
                                  fragments=int(size.n_frags), out_text_bytes=int(size.text_bytes), item_text_bytes=int(toffs[-1]),
                                  scanned_bytes=scanned, highlight_call_ms=round(call_ms, 3), count_part_ms=round(count_ms, 3),
                                  emit_part_ms=round(float(np.mean(emit)), 3),
                                  scanned_GBps_whole_call=round(scanned / call_ms / 1e6, 1),
                                  scanned_GBps_count_part=round(scanned / count_ms / 1e6, 1),
                                  share_of_hbm_peak_whole_call=round(scanned / (call_ms * 1e-3) / HBM_PEAK, 5),
                                  host_16_threads_ms=round(cpu16, 2), host_over_device=round(cpu16 / call_ms, 2))), flush=True)
        del keep
    ix.close()

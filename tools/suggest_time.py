"""Time of the completion suggester (slg_suggest_batch) over the vocabulary of tools/expand_time.py (2^18 generated
words, Zipf-like doc frequencies 200000 / (rank + 1)), as ONE segment and as THREE (segment s holds the words of
rank r with (r + s) % 3 != 0: every word in two of them), and batches of 4096 requests of size 5:
  * plain: the first 1 .. 4 chars of a random word (the four lengths in turn);
  * fuzzy: a random word under the default FuzzyOptions (1 edit, 50 expansions, min length 3) at prefix_length 1,
    then the same at prefix_length 0.
Per batch, mean of `reps` calls after two warm-up calls, `rounds` times over so the spread shows:
  * slg_suggest_batch: the whole call by the host clock (the call ends in a stream synchronise), and its own split
    into the device part (uploads, scan + merge kernels, the copy back, the wait) and the host's copy of the texts
    (slg_suggest_phase_ms);
  * the same requests by the C++ restatement of the reference's loop (csrc/slg_suggest_capi.cpp,
    slgx_reference_suggest) on this box, at 1 and 16 threads; the 1-thread prefix-0 figure is timed on every 8th
    request and multiplied by 8 (stated in the line).
The device's answer is compared with the restatement's, bit for bit, before anything is timed.
usage (GPU box): python tools/suggest_time.py [reps] [rounds]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from searchlite_amd import build, searcher, _native as N  # noqa: E402
from searchlite_amd.segment import Segment  # noqa: E402
from tools.vocabulary import make_vocabulary  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
vocab, n_reqs, size = 1 << 18, 4096, 5

L = C.CDLL(build.build_plan_lib())
L.slgx_dict_build.restype = C.c_void_p
L.slgx_dict_build.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint32, C.c_void_p]
L.slgx_dict_tables.restype = C.c_uint32
L.slgx_dict_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
L.slgx_reference_suggest.restype = C.c_int
L.slgx_reference_suggest.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                     C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_char_p,
                                     C.c_uint32]
err = C.create_string_buffer(256)


def df_segment(keys, dfs):
    offs = np.zeros(len(keys) + 1, dtype=np.uint64)
    np.cumsum(dfs, out=offs[1:])
    n_docs = int(dfs.max())
    total = int(offs[-1])
    doc_ids = (np.arange(total, dtype=np.uint64) - np.repeat(offs[:-1], dfs.astype(np.int64))).astype(np.uint32)   # list t: docs 0 .. df - 1
    return Segment(n_docs=n_docs, term_offsets=offs, doc_ids=doc_ids, tfs=np.ones(total, np.uint32),
                   field_doc_len=[np.ones(n_docs, np.float32)], field_avgdl=np.ones(1, np.float32), docs=float(n_docs))


def host_dict(keys, dfs):
    """the library's host dictionary of a segment and its df in sorted-position order"""
    raw = [k.encode() for k in keys]
    koffs = np.zeros(len(raw) + 1, dtype=np.uint32)
    np.cumsum([len(r) for r in raw], out=koffs[1:])
    blob = np.frombuffer(b"".join(raw), dtype=np.uint8)
    hd = L.slgx_dict_build(len(raw), blob.ctypes.data, koffs.ctypes.data, err, 256, None)
    assert hd, err.value
    order = np.zeros(len(raw), dtype=np.uint32)
    L.slgx_dict_tables(hd, order.ctypes.data, None)
    return hd, np.ascontiguousarray(dfs[order].astype(np.uint32))


def c_reqs(reqs):
    keep = []
    arr = (N.SuggestReq * len(reqs))()
    for i, r in enumerate(reqs):
        f, t = r["field"].encode(), r["term"].encode()
        keep += [f, t]
        fz = r["fuzzy"] or dict(max_edits=0, prefix_length=0, max_expansions=0, min_length=0)
        arr[i] = N.SuggestReq(C.sizeof(N.SuggestReq), f, t, len(f), len(t), r["size"], 0 if r["fuzzy"] is None else 1,
                              fz["max_edits"], fz["prefix_length"], fz["max_expansions"], fz["min_length"])
    return arr, keep


t0 = time.time()
words = make_vocabulary(vocab)
all_dfs = np.maximum(1, 200000 // (np.arange(vocab, dtype=np.int64) + 1)).astype(np.uint64)
rng = np.random.default_rng(11)
picks = rng.integers(0, vocab, size=n_reqs)
batches = [("plain_prefix_1_to_4_chars", [searcher.suggest_request("body", words[int(t)][:1 + i % 4], size)
                                          for i, t in enumerate(picks)])]
for pl in (1, 0):
    batches.append((f"fuzzy_prefix_length_{pl}", [searcher.suggest_request("body", words[int(t)], size, dict(prefix_length=pl))
                                                  for t in picks]))

for n_segs in (1, 3):
    if n_segs == 1:
        parts = [np.arange(vocab)]
    else:
        parts = [np.array([r for r in range(vocab) if (r + s) % 3 != 0]) for s in range(3)]
    seg_keys = [["body:" + words[int(r)] for r in part] for part in parts]
    ix = searcher.GpuIndex([df_segment(k, all_dfs[part]) for k, part in zip(seg_keys, parts)])
    ix.set_stream(torch.cuda.current_stream().cuda_stream)
    hosts = []
    for s, (k, part) in enumerate(zip(seg_keys, parts)):
        ix.set_terms(s, k)
        hosts.append(host_dict(k, all_dfs[part]))
    dicts = (C.c_void_p * n_segs)(*[h for h, _ in hosts])
    dfs = (C.c_void_p * n_segs)(*[d.ctypes.data for _, d in hosts])
    print(json.dumps(dict(vocabulary=vocab, segments=n_segs, keys_per_segment=[len(k) for k in seg_keys],
                          requests=n_reqs, size=size, setup_s=round(time.time() - t0, 1))), flush=True)

    def host_loop(reqs, n_threads, want=False):
        arr, keep = c_reqs(reqs)
        o = np.zeros(len(reqs) + 1, dtype=np.uint32)
        cap, tcap = len(reqs) * size, len(reqs) * size * 16
        sc, df = (np.zeros(cap, np.float32), np.zeros(cap, np.uint64)) if want else (None, None)
        to, tx = (np.zeros(cap + 1, np.uint32), np.zeros(tcap, np.uint8)) if want else (None, None)
        p = lambda a: None if a is None else a.ctypes.data
        t = time.perf_counter()
        rc = L.slgx_reference_suggest(dicts, dfs, n_segs, arr, len(reqs), n_threads, o.ctypes.data, cap, p(sc), p(df), p(to),
                                      tcap, p(tx), err, 256)
        ms = (time.perf_counter() - t) * 1e3
        assert rc == 0, err.value
        return ms, o, sc, df, to, tx

    for name, reqs in batches:
        arr, keep = c_reqs(reqs)
        cap, tcap = n_reqs * size, n_reqs * size * 16
        o, sc, df = np.zeros(n_reqs + 2, np.uint32), np.zeros(cap, np.float32), np.zeros(cap, np.uint64)
        to, tx = np.zeros(cap + 1, np.uint32), np.zeros(tcap, np.uint8)

        def one_call():
            N.check(ix._lib.slg_suggest_batch(ix._h, arr, n_reqs, o.ctypes.data, cap, sc.ctypes.data, df.ctypes.data,
                                              to.ctypes.data, tcap, tx.ctypes.data))
        one_call()
        _, ro, rsc, rdf, rto, rtx = host_loop(reqs, 16, want=True)      # the same answer before any timing
        n = int(ro[-1])
        assert o[:n_reqs + 1].tolist() == ro.tolist() and sc[:n].view(np.uint32).tolist() == rsc[:n].view(np.uint32).tolist()
        assert df[:n].tolist() == rdf[:n].tolist() and to[:n + 1].tolist() == rto[:n + 1].tolist()
        assert tx[:int(to[n])].tobytes() == rtx[:int(rto[n])].tobytes()
        one_call()
        for rnd in range(rounds):
            call, dev, copy = [], [], []
            for _ in range(reps):
                t = time.perf_counter()
                one_call()
                call.append((time.perf_counter() - t) * 1e3)
                d, c = ix.suggest_phase_ms()
                dev.append(d)
                copy.append(c)
            sub = reqs[::8] if name.endswith("_0") else reqs
            cpu1 = host_loop(sub, 1)[0] * (len(reqs) / len(sub))
            cpu16 = host_loop(reqs, 16)[0]
            print(json.dumps(dict(segments=n_segs, batch=name, round=rnd, requests=n_reqs, options=n,
                                  suggest_call_ms=round(float(np.mean(call)), 3), device_ms=round(float(np.mean(dev)), 3),
                                  host_text_copy_ms=round(float(np.mean(copy)), 3), cpu_loop_1_thread_ms=round(cpu1, 1),
                                  cpu_1_thread_timed_on="every 8th request, x8" if len(sub) != len(reqs) else "all requests",
                                  cpu_loop_16_threads_ms=round(cpu16, 2))), flush=True)
    ix.close()

"""Counting the guides of 10 M resident reads against their KNOWN library, one substitution tolerated: the device route (inserts_tensor,
tally_library, the table copied to the host, library_counts) against the plain tally of the same spans, and against the route a caller
had before the library tally -- the plain tally, its table to the host, an exact look-up of the library's keys and a NumPy walk of the
3 L neighbours of every distinct key that is no entry.
Usage (GPU box): python3 profiles/tally_library_bench.py [--lines N] [--distinct M] [--guides G] [--runs K]
  -> one JSON line, appended to profiles/tally_library_bench.jsonl.
Input: the grouped-tally benchmark's (tally_grouped_bench.py: N x 150 bp lines, M distinct lines tiled on the device, about 90 % of them
with flank A + a 20-base guide (one of G) + flank B ...), with ONE SUBSTITUTION planted in about 10 % of the guides.  The scanner
profiles, so the tallies' own HIP-event times (last_tally_ms) are recorded beside the wall times.  Best of K timed runs (after one
untimed run); the host route runs once.  Both routes must give the same dense count vector."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from seeq_amd import device as dev
from inserts_bench import L, best_of
from tally_grouped_bench import ACGT, FA, FB, FC, FD, GUIDE, SPACER, UMI, keys_of


def make_lines(m, nguides, seed, error_rate=0.1):
    """m lines of L bases + newline as one uint8 array, and the library (nguides x GUIDE bases)."""
    rng = np.random.default_rng(seed)
    a = ACGT[rng.integers(0, 4, size=(m, L + 1))]
    a[:, L] = 10
    planted = np.nonzero(rng.random(m) < 0.9)[0]
    span = 4 * 20 + GUIDE + UMI + SPACER
    col = rng.integers(3, L - span - 3, size=planted.size)
    code = rng.integers(0, 4, size=(nguides, GUIDE))
    which = rng.integers(0, nguides, size=planted.size)
    guide = code[which]
    bad = np.nonzero(rng.random(planted.size) < error_rate)[0]      # one substitution: another base at one position
    at = rng.integers(0, GUIDE, size=bad.size)
    guide[bad, at] = (guide[bad, at] + rng.integers(1, 4, size=bad.size)) % 4
    off = 0
    for part in (FA, ACGT[guide], FB, None, FC, None, FD):
        if part is None:
            off += SPACER if off == 3 * 20 else UMI
            continue
        block = np.frombuffer(part.encode(), dtype=np.uint8)[None, :] if isinstance(part, str) else part
        for i in range(block.shape[1]):
            a[planted, col + off + i] = block[:, i]
        off += block.shape[1]
    assert off == span
    return a.reshape(-1), ACGT[code]


def host_route(sc, t, lib_keys):
    """What a caller did before: the plain tally, its table to the host, the library's keys looked up exactly, and for every distinct key
    that is no entry its 3 L neighbours looked up in NumPy -> the dense count vector."""
    res = sc.tally(t)
    keys, counts = res["keys"], res["counts"]
    order = np.argsort(lib_keys)
    skey = lib_keys[order]

    def find(q):                                            # -> index into the library, -1: no entry
        at = np.minimum(np.searchsorted(skey, q), len(skey) - 1)
        return np.where(skey[at] == q, order[at], -1)
    dense = np.zeros(len(lib_keys), dtype=np.uint64)
    exact = find(keys)
    np.add.at(dense, exact[exact >= 0], counts[exact >= 0])
    rest, rcount = keys[exact < 0], counts[exact < 0]
    length = (np.floor(np.log2(rest.astype(np.float64))).astype(np.int64)) // 2
    nfound = np.zeros(len(rest), dtype=np.int64)
    which = np.zeros(len(rest), dtype=np.int64)
    for p in range(int(length.max()) if len(rest) else 0):
        ok = length > p
        for s in (1, 2, 3):
            hit = find(rest ^ (np.uint64(s) << (np.uint64(2) * (length - 1 - p).clip(0).astype(np.uint64))))
            hit[~ok] = -1
            nfound += hit >= 0
            which = np.where(hit >= 0, hit, which)
    one = nfound == 1
    np.add.at(dense, which[one], rcount[one])
    return dense, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--distinct", type=int, default=1_000_000)
    ap.add_argument("--guides", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "tally_library_bench.jsonl"))
    args = ap.parse_args()
    distinct = min(args.distinct, args.lines)
    torch.cuda.set_device(0)
    lines, library = make_lines(distinct, args.guides, 31)
    t = torch.from_numpy(lines).cuda().repeat(max(1, args.lines // distinct))
    nlines = t.numel() // (L + 1)
    lib_keys = keys_of(library)
    assert len(np.unique(lib_keys)) == len(lib_keys), "the random library holds a duplicate: another seed"
    pats = [dev.Pattern(f, 0) for f in (FA, FB)]
    sc = dev.Scanner()
    sc.set_profiling(True)
    sc.set_library(lib_keys, 1)
    state = {}

    def device_route():
        state["ins"] = sc.inserts_tensor(pats[0], pats[1], t, dev.SQ_BEST, copy=False)
        return sc.tally_library(t)
    t_dev, res = best_of(device_route, args.runs)
    t_lib, lazy = best_of(lambda: sc.tally_library(t, copy=False), args.runs)
    lib_event_ms = sc.last_tally_ms()
    sc.set_library(lib_keys, 0)
    t_lib0, lazy0 = best_of(lambda: sc.tally_library(t, copy=False), args.runs)
    lib0_event_ms = sc.last_tally_ms()
    sc.set_library(lib_keys, 1)
    t_plain, plain = best_of(lambda: sc.tally(t, copy=False), args.runs)      # the plain tally of the same spans
    plain_event_ms = sc.last_tally_ms()
    dense = dev.library_counts(res, len(lib_keys))
    torch.cuda.synchronize(); t0 = time.perf_counter()
    sc.inserts_tensor(pats[0], pats[1], t, dev.SQ_BEST, copy=False)
    host_dense, host_plain = host_route(sc, t, lib_keys)
    t_host = time.perf_counter() - t0
    same = bool(np.array_equal(dense, host_dense)) and int(dense.sum()) == res["nassigned"] and state["ins"]["ninserts"] == res["nspans"] == plain["nspans"]
    assert same, "the two routes differ"
    names = ("nspans", "nassigned", "nexact", "ncorrected", "nambiguous", "nunknown", "nlong", "nforeign", "ndistinct", "key_bits", "passes")
    row = {"lines": nlines, "read_len": L, "text_bytes_scanned": t.numel(), "guides": args.guides, "counts": {k: res[k] for k in names},
           "library_tally_event_ms": round(lib_event_ms, 3), "library_tally_wall_ms": round(t_lib * 1e3, 3),
           "exact_only_event_ms": round(lib0_event_ms, 3), "exact_only_wall_ms": round(t_lib0 * 1e3, 3), "exact_only_assigned": lazy0["nassigned"],
           "plain_tally_event_ms": round(plain_event_ms, 3), "plain_tally_wall_ms": round(t_plain * 1e3, 3), "plain_tally_passes": plain["passes"],
           "plain_tally_distinct": plain["ndistinct"], "device_route_ms": round(t_dev * 1e3, 3), "host_route_ms": round(t_host * 1e3, 3),
           "host_over_device": round(t_host / t_dev, 1), "identical": same}
    print(json.dumps(row), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")
    sc.close()


if __name__ == "__main__":
    main()

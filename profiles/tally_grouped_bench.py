"""Counting the distinct (guide, UMI) pairs of 10 M resident reads: the device route (inserts_tensor, tally_hold, inserts_tensor,
tally_grouped, both tables copied to the host) against the route a caller had before the grouped tally -- two inserts_tensor calls with
their records, both insert texts copied to the host, the join by line and np.unique over the joined pairs in NumPy.
Usage (GPU box): python3 profiles/tally_grouped_bench.py [--lines N] [--distinct M] [--guides G] [--runs K]
  -> one JSON line, appended to profiles/tally_grouped_bench.jsonl.
Input: N x 150 bp lines (M distinct lines tiled on the device), about 90 % of them with flank A + a 20-base guide (one of G) + flank B,
five bases, flank C + a 12-base UMI + flank D; the four 20-mer flanks are planted exactly and searched at distance 0 under SQ_BEST.  The
device route is timed with profiling on, so the grouped call's own HIP-event time (last_tally_grouped_ms) is recorded beside the wall
times of the hold alone, of the grouped call alone (tables left on the device), of the two table copies and of the whole route.  Best of
K timed runs (after one untimed run); the host route runs once.  Both routes must give the same two tables: the host's distinct pairs
are keyed by the rule of seeq_tally.h in NumPy and ordered by (group, member)."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from seeq_amd import device as dev
from inserts_bench import L, best_of

FA, FB = "GATGTAGCGCGATTAGCCTG", "TTCACTGGAGTTGTCCCAAT"
FC, FD = "CCGATAGGCTTAACGGTCAC", "AGGTCCATTGCAGTACGGAT"
GUIDE, UMI, SPACER = 20, 12, 5
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def make_lines(m, nguides, seed):
    """m lines of L bases + newline as one uint8 array."""
    rng = np.random.default_rng(seed)
    a = ACGT[rng.integers(0, 4, size=(m, L + 1))]
    a[:, L] = 10
    planted = np.nonzero(rng.random(m) < 0.9)[0]
    span = 4 * 20 + GUIDE + UMI + SPACER
    col = rng.integers(3, L - span - 3, size=planted.size)
    library = ACGT[rng.integers(0, 4, size=(nguides, GUIDE))]
    guide = library[rng.integers(0, nguides, size=planted.size)]
    at = 0
    for part in (FA, guide, FB, None, FC, None, FD):
        if part is None:                                    # the spacer, then the UMI: the random bases that are there
            at += SPACER if at == 3 * 20 else UMI
            continue
        block = np.frombuffer(part.encode(), dtype=np.uint8)[None, :] if isinstance(part, str) else part
        for i in range(block.shape[1]):
            a[planted, col + at + i] = block[:, i]
        at += block.shape[1]
    assert at == span
    return a.reshape(-1)


def host_route(sc, pats, t):
    """What a caller did before the grouped tally: two inserts calls, their records and insert texts to the host, the join by line and
    np.unique over the joined (guide, UMI) byte rows there."""
    g = sc.inserts_tensor(pats[0], pats[1], t, dev.SQ_BEST)
    gtext = sc.insert_text(t).cpu().numpy()
    u = sc.inserts_tensor(pats[2], pats[3], t, dev.SQ_BEST)
    utext = sc.insert_text(t).cpu().numpy()
    assert gtext.size == g["ninserts"] * (GUIDE + 1) and utext.size == u["ninserts"] * (UMI + 1), "this input's inserts have one length each"
    _, gi, ui = np.intersect1d(g["records"]["line"], u["records"]["line"], assume_unique=True, return_indices=True)
    rows = np.concatenate((gtext.reshape(-1, GUIDE + 1)[gi, :GUIDE], utext.reshape(-1, UMI + 1)[ui, :UMI]), axis=1)
    pairs, counts = np.unique(np.ascontiguousarray(rows).view("V%d" % (GUIDE + UMI)).reshape(-1), return_counts=True)
    return pairs, counts, g["ninserts"], u["ninserts"]


def keys_of(a):
    """Rows of bases -> their tally keys."""
    key = np.ones(len(a), dtype=np.uint64)
    for j in range(a.shape[1]):
        key = (key << np.uint64(2)) | ((a[:, j] >> 1) & 3).astype(np.uint64)
    return key


def tables_of(pairs, counts):
    """The host's distinct byte rows and their counts -> the two tables by the rule."""
    a = np.frombuffer(pairs.tobytes(), dtype=np.uint8).reshape(len(pairs), GUIDE + UMI)
    gk, mk = keys_of(a[:, :GUIDE]), keys_of(a[:, GUIDE:])
    order = np.lexsort((mk, gk))
    ptab = np.zeros(len(pairs), dtype=dev.TALLY_PAIR_DTYPE)
    ptab["group"], ptab["member"], ptab["count"] = gk[order], mk[order], counts[order]
    heads = np.nonzero(np.concatenate(([True], ptab["group"][1:] != ptab["group"][:-1])))[0] if len(ptab) else np.zeros(0, dtype=np.int64)
    gtab = np.zeros(len(heads), dtype=dev.TALLY_GROUP_DTYPE)
    if len(heads):
        gtab["group"], gtab["first"] = ptab["group"][heads], heads
        gtab["count"] = np.add.reduceat(ptab["count"], heads)
        gtab["ndistinct"] = np.diff(np.concatenate((heads, [len(ptab)])))
    return ptab, gtab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--distinct", type=int, default=1_000_000)
    ap.add_argument("--guides", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "tally_grouped_bench.jsonl"))
    args = ap.parse_args()
    distinct = min(args.distinct, args.lines)
    torch.cuda.set_device(0)
    t = torch.from_numpy(make_lines(distinct, args.guides, 31)).cuda().repeat(max(1, args.lines // distinct))
    nlines = t.numel() // (L + 1)
    pats = [dev.Pattern(f, 0) for f in (FA, FB, FC, FD)]
    sc = dev.Scanner()
    sc.set_profiling(True)
    state = {}

    def device_route():
        state["g"] = sc.inserts_tensor(pats[0], pats[1], t, dev.SQ_BEST, copy=False)
        state["hold"] = sc.tally_hold(t)
        state["u"] = sc.inserts_tensor(pats[2], pats[3], t, dev.SQ_BEST, copy=False)
        return sc.tally_grouped(t)
    t_dev, res = best_of(device_route, args.runs)
    grouped_event_ms = sc.last_tally_grouped_ms()
    t_grouped, lazy = best_of(lambda: sc.tally_grouped(t, copy=False), args.runs)
    t_copy, _ = best_of(lambda: (sc.tally_pairs_table(lazy["npairs"]), sc.tally_groups_table(lazy["ngroups"])), args.runs)
    t_plain, plain = best_of(lambda: sc.tally(t, copy=False), args.runs)      # the plain tally of the same spans (the UMIs), for scale
    plain_event_ms = sc.last_tally_ms()
    sc.inserts_tensor(pats[0], pats[1], t, dev.SQ_BEST, copy=False)
    t_hold, _ = best_of(lambda: sc.tally_hold(t), args.runs)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    pairs, counts, ng, nu = host_route(sc, pats, t)
    t_host = time.perf_counter() - t0
    ptab, gtab = tables_of(pairs, counts)
    same = (ptab.tobytes() == res["pairs"].tobytes() and gtab.tobytes() == res["groups"].tobytes() and int(counts.sum()) == res["npaired"]
            and (ng, nu) == (state["g"]["ninserts"], state["u"]["ninserts"]) == (state["hold"]["nspans"], res["nspans"]))
    assert same, "the two routes differ"
    row = {"lines": nlines, "read_len": L, "text_bytes_scanned": t.numel(), "guides": args.guides,
           "hold": {k: state["hold"][k] for k in ("nspans", "nheld", "nlong", "nforeign", "max_len", "key_bits")},
           "counts": {k: res[k] for k in ("nspans", "npaired", "nlong", "nforeign", "nungrouped", "npairs", "ngroups", "max_len", "passes")},
           "grouped_event_ms": round(grouped_event_ms, 3), "grouped_wall_ms": round(t_grouped * 1e3, 3), "hold_wall_ms": round(t_hold * 1e3, 3),
           "tables_copy_ms": round(t_copy * 1e3, 3), "plain_tally_event_ms": round(plain_event_ms, 3), "plain_tally_passes": plain["passes"],
           "device_route_ms": round(t_dev * 1e3, 3), "host_route_ms": round(t_host * 1e3, 3), "host_over_device": round(t_host / t_dev, 1),
           "identical": same}
    print(json.dumps(row), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")
    sc.close()


if __name__ == "__main__":
    main()

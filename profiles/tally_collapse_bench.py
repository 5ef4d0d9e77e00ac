"""Collapsing the UMI errors of the (guide, UMI) pairs of 10 M resident reads: the device route (tally_collapse behind tally_grouped, its
parents and group rows copied to the host) against the route a caller had before it -- both tables of the grouped tally copied to the
host and a NumPy walk of the 3 L neighbours of every pair within its group.
Usage (GPU box): python3 profiles/tally_collapse_bench.py [--lines N] [--distinct M] [--guides G] [--runs K]
  -> one JSON line, appended to profiles/tally_collapse_bench.jsonl.
Input: the grouped-tally benchmark's (tally_grouped_bench.py: N x 150 bp lines, M distinct lines tiled on the device, about 90 % of them
with flank A + a 20-base guide (one of G) + flank B, five bases, flank C + a 12-base UMI + flank D), with ONE SUBSTITUTION planted, after
the tiling, in about 10 % of the UMIs: a distinct line's UMI then stands about nine times as it was and about once with an error.  The
scanner profiles, so the collapse's and the grouped call's own HIP-event times (last_tally_collapse_ms, last_tally_grouped_ms) are
recorded beside the wall times.  Best of K timed runs (after one untimed run); the host route runs once.  Both routes must give the same
parents and the same group rows, under both rules."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from seeq_amd import device as dev
from inserts_bench import L, best_of
from tally_grouped_bench import ACGT, FA, FB, FC, FD, GUIDE, SPACER, UMI

RULES = ("directional", "any")


def make_lines(m, nguides, seed):
    """tally_grouped_bench.make_lines, which also says where a line's UMI lies: (text, planted lines, the column of their UMI)."""
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
    return a.reshape(-1), planted, col + 3 * 20 + GUIDE + SPACER


def plant_errors(t, distinct, planted, umi_col, seed, rate=0.1):
    """One substitution in about `rate` of the UMIs of the tiled text t, in place on the device; -> how many."""
    nlines = t.numel() // (L + 1)
    rng = np.random.default_rng(seed)
    where = np.full(distinct, -1, dtype=np.int64)
    where[planted] = umi_col
    rows = np.nonzero(rng.random(nlines) < rate)[0]
    rows = rows[where[rows % distinct] >= 0]
    at = rows * (L + 1) + where[rows % distinct] + rng.integers(0, UMI, size=rows.size)
    at = torch.from_numpy(at).cuda()
    step = torch.from_numpy(rng.integers(1, 4, size=rows.size)).cuda()
    lut = torch.zeros(256, dtype=torch.int64, device="cuda")
    lut[torch.from_numpy(ACGT.copy()).cuda().long()] = torch.arange(4, device="cuda")
    t[at] = torch.from_numpy(ACGT.copy()).cuda()[(lut[t[at].long()] + step) % 4]
    return int(rows.size)


def host_route(sc, npairs, ngroups):
    """What a caller did before: both tables to the host, and per pair its 3 L neighbours looked up among the pairs of its group in NumPy ->
    {rule: (parent, group rows)}."""
    pairs, groups = sc.tally_pairs_table(npairs), sc.tally_groups_table(ngroups)
    m, c = pairs["member"], pairs["count"]
    length = (np.floor(np.log2(m.astype(np.float64))).astype(np.int64)) // 2
    assert int(length.max()) <= 15, "the walk packs (group rank, member) into one 64-bit search key: members of at most 15 bases"
    rank = np.repeat(np.arange(ngroups, dtype=np.uint64), groups["ndistinct"].astype(np.int64))
    skey = (rank << np.uint64(32)) | m                      # ascending, as the table is
    idx = np.arange(npairs, dtype=np.int64)
    best = {rule: [np.zeros(npairs, dtype=np.uint64), np.zeros(npairs, dtype=np.uint64), np.full(npairs, -1, dtype=np.int64)] for rule in RULES}
    for p in range(int(length.max())):
        ok = length > p
        shift = (np.uint64(2) * (length - 1 - p).clip(0).astype(np.uint64))
        for s in (1, 2, 3):
            nb = m ^ (np.uint64(s) << shift)
            j = np.minimum(np.searchsorted(skey, (rank << np.uint64(32)) | nb), npairs - 1)
            found = ok & (skey[j] == ((rank << np.uint64(32)) | nb))
            cj = c[j]
            pre = found & ((cj > c) | ((cj == c) & (nb < m)))
            for rule in RULES:
                bc, bm, bj = best[rule]
                cand = pre if rule == "any" else pre & ((cj - np.minimum(c, cj)) >= (c - np.uint64(1)))
                better = cand & ((bj < 0) | (cj > bc) | ((cj == bc) & (nb < bm)))
                bc[better], bm[better], bj[better] = cj[better], nb[better], j[better]
    out = {}
    first = groups["first"].astype(np.int64)
    for rule in RULES:
        bj = best[rule][2]
        parent = np.where(bj >= 0, bj, idx).astype(np.uint32)
        absorbed = parent != idx
        rows = np.zeros(ngroups, dtype=dev.TALLY_COLLAPSE_DTYPE)
        rows["nabsorbed"] = np.add.reduceat(absorbed.astype(np.int64), first)
        rows["nroots"] = groups["ndistinct"] - rows["nabsorbed"]
        rows["absorbed_reads"] = np.add.reduceat(np.where(absorbed, c, np.uint64(0)), first)
        out[rule] = (parent, rows)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--distinct", type=int, default=1_000_000)
    ap.add_argument("--guides", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "tally_collapse_bench.jsonl"))
    args = ap.parse_args()
    distinct = min(args.distinct, args.lines)
    torch.cuda.set_device(0)
    lines, planted, umi_col = make_lines(distinct, args.guides, 31)
    t = torch.from_numpy(lines).cuda().repeat(max(1, args.lines // distinct))
    nlines = t.numel() // (L + 1)
    nerrors = plant_errors(t, distinct, planted, umi_col, 32)
    pats = [dev.Pattern(f, 0) for f in (FA, FB, FC, FD)]
    sc = dev.Scanner()
    sc.set_profiling(True)
    sc.inserts_tensor(pats[0], pats[1], t, dev.SQ_BEST, copy=False)
    hold = sc.tally_hold(t)
    sc.inserts_tensor(pats[2], pats[3], t, dev.SQ_BEST, copy=False)
    t_grouped, grouped = best_of(lambda: sc.tally_grouped(t, copy=False), args.runs)
    grouped_event_ms = sc.last_tally_grouped_ms()
    device, event_ms, wall_ms, copy_ms = {}, {}, {}, {}
    for rule in RULES:
        t_lazy, lazy = best_of(lambda: sc.tally_collapse(rule, copy=False), args.runs)
        event_ms[rule], wall_ms[rule] = round(sc.last_tally_collapse_ms(), 3), round(t_lazy * 1e3, 3)
        t_copy, tabs = best_of(lambda: (sc.tally_parents_table(lazy["npairs"]), sc.tally_collapse_table(lazy["ngroups"])), args.runs)
        copy_ms[rule] = round(t_copy * 1e3, 3)
        device[rule] = (lazy, tabs)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    host = host_route(sc, grouped["npairs"], grouped["ngroups"])
    t_host = time.perf_counter() - t0
    same = all(np.array_equal(device[r][1][0], host[r][0]) and device[r][1][1].tobytes() == host[r][1].tobytes() and
               device[r][0]["nroots"] == int(host[r][1]["nroots"].sum()) and device[r][0]["absorbed_reads"] == int(host[r][1]["absorbed_reads"].sum())
               for r in RULES)
    assert same, "the two routes differ"
    names = ("npairs", "ngroups", "nroots", "nabsorbed", "absorbed_reads", "rule", "max_len")
    t_dev = sum(wall_ms[r] + copy_ms[r] for r in RULES) / 1e3
    row = {"lines": nlines, "read_len": L, "text_bytes_scanned": t.numel(), "guides": args.guides, "umi_errors_planted": nerrors, "held": hold["nheld"],
           "grouped": {k: grouped[k] for k in ("nspans", "npaired", "npairs", "ngroups", "max_len", "passes")},
           "grouped_event_ms": round(grouped_event_ms, 3), "grouped_wall_ms": round(t_grouped * 1e3, 3),
           "counts": {r: {k: device[r][0][k] for k in names} for r in RULES},
           "collapse_event_ms": event_ms, "collapse_wall_ms": wall_ms, "copy_ms": copy_ms,
           "device_route_both_rules_ms": round(t_dev * 1e3, 3), "host_route_both_rules_ms": round(t_host * 1e3, 3),
           "host_over_device": round(t_host / t_dev, 1), "identical": same}
    print(json.dumps(row), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")
    sc.close()


if __name__ == "__main__":
    main()

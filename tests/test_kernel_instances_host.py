"""The ledger of kernel instances (tests/kernel_instances.py), checked without a GPU: every template instance of the scan kernels and of the
post-pass that the planner (seeq_amd/csrc/seeq_plan.h) can select has a row in REPRESENTATIVES -- the scan tests/test_gpu_kernel_instances.py
runs against the oracle -- and what is compiled but never selected is listed as UNREACHABLE, with the reason."""
import time

import numpy as np
import pytest

import kernel_instances as K


@pytest.fixture(scope="module")
def census_all(harness):
    K.use_harness(harness)
    t0 = time.time()
    found = K.census_all()
    print("census: %d keys in %.1f s" % (len(found), time.time() - t0))
    return found


@pytest.fixture(scope="module")
def census(census_all):
    return K.census(census_all)


@pytest.fixture(scope="module")
def rows():
    return K.rows()


def _predicted(rows):
    """key of every row from the planner over the row's inputs -- the rows of one (pattern, tau) planned together"""
    H = K.harness_lib()
    groups = {}
    for i, r in enumerate(rows):
        groups.setdefault((r.pattern, r.tau), []).append(i)
    keys = [None] * len(rows)
    for (expr, tau), idx in groups.items():
        grid = np.array([(rows[i].options, rows[i].want, rows[i].flags, rows[i].kernel) for i in idx], dtype=np.int32)
        out = K.plans_of(H, expr, tau, grid, [rows[i].avg_line for i in idx])
        for i, o in zip(idx, out):
            keys[i] = K.instance_key(dict(zip(K.PLAN_FIELDS, (int(v) for v in o))), rows[i].options, rows[i].want)
    return keys


def ledger_gaps(census, rows, predicted):
    """What is wrong with the ledger -> list of lines (empty: complete)"""
    out = []
    have = {r.key for r in rows}
    for key in sorted(set(census) - have):
        inp = census[key]
        out.append("no row for %s -- reached by %s" % (key, K._row_of(key, inp).line().strip()))
    for r, got in zip(rows, predicted):
        if got != r.key:
            out.append("the row of %s runs %s" % (r.key, got))
    for key in sorted(have - set(census)):
        out.append("a row for %s, which the census does not reach" % key)
    if len(have) != len(rows):
        out.append("%d rows for %d keys: one row per key" % (len(rows), len(have)))
    return out


def test_every_reachable_instance_has_a_representative(census, rows):
    """Ledger complete: every key of the census (lengths 4 ... 62 and the two class patterns x tau <= min(m - 1, 15) x non-DNA mode x FASTA x
    four line lengths x SEEQ_FUSED_KERNEL x the context's flags x four (match, want) pairs: 1.2 million plans, the automata of a (pattern, tau)
    built once -- 20 s, 14 of them the automata) has a row, and every row's key is what the planner gives for the row's inputs.  A failure
    lists each missing key with a row that reaches it.  Rows that need a knob are there only where no plain scan reaches the key."""
    predicted = _predicted(rows)
    gaps = ledger_gaps(census, rows, predicted)
    assert not gaps, "\n" + "\n".join(gaps)
    level = {key: (inp["kernel"] != 0) for key, inp in census.items()}
    for r in rows:
        assert bool(r.knobs) == level[r.key], "%s: knobs %r, but the census reaches it %s one" % (r.key, r.knobs, "only with" if level[r.key] else "without")
    print("%d keys, %d reached without a knob" % (len(rows), sum(1 for r in rows if not r.knobs)))


def test_the_ledger_test_names_what_is_missing(census, rows):
    """A key nobody has a row for, and a row taken out: the gaps name the instance and an input that reaches it."""
    predicted = _predicted(rows)
    fake = "k_pair<9,plain> | order2 | k_verify<1,BEST,vr?>+k_emit1"
    inp = dict(pattern="GATGTAGCGCGATTAGCCTG", tau=3, options=K.SQ_BEST, want=K.RECORDS, avg_line=151.0, flags=0, kernel=0)
    gaps = ledger_gaps(dict(census, **{fake: inp}), rows, predicted)
    assert len(gaps) == 1 and fake in gaps[0] and "GATGTAGCGCGATTAGCCTG" in gaps[0], gaps
    gaps = ledger_gaps(census, rows[:7] + rows[8:], predicted[:7] + predicted[8:])
    assert len(gaps) == 1 and rows[7].key in gaps[0] and gaps[0].startswith("no row for"), gaps
    # a row whose inputs run another instance than it claims
    wrong = K.Row(rows[0].key, rows[1].pattern, rows[1].tau, K.options_text(rows[1].options), K.WANT_NAMES[rows[1].want], rows[1].avg_line, rows[1].recipe,
                  rows[1].knobs)
    gaps = ledger_gaps(census, [wrong] + rows[1:], _predicted([wrong]) + predicted[1:])
    assert any(g.startswith("the row of " + rows[0].key) for g in gaps), gaps


def test_compiled_instances_are_reached_or_listed_unreachable(census):
    """Every instance the dispatch code names (kernel_instances.COMPILED) appears in a key of the census or in UNREACHABLE -- never both: the
    census really does not produce what UNREACHABLE lists."""
    keys = [k + " |" for k in census]
    unreachable = [u for u, why in K.UNREACHABLE]
    assert all(why for u, why in K.UNREACHABLE)
    for u in unreachable:
        assert u in K.COMPILED, u
        assert not [k for k in keys if u in k], (u, [k for k in keys if u in k][:3])
    lost = [c for c in K.COMPILED if c not in unreachable and not any(c in k for k in keys)]
    assert not lost, "compiled, not reached by the census and not in UNREACHABLE: %s" % lost
    # and the census runs nothing the list of compiled instances does not know: the scan kernel of every key
    scans = {k.split(" | ")[0].split("+ll_filter")[0] for k in census}
    assert scans <= set(K.COMPILED) | {"k_forward"}, scans - set(K.COMPILED)


def test_the_row_maker_picks_rows_that_run_their_key_and_pass_the_oracle(census_all, census, oracle):
    """What writes tests/kernel_instance_rows.py: the row made of ANY census input runs the key it was found for, and choose_rows, let loose on
    the keys two (pattern, tau) pairs reach, gives each a row at the key's level whose text the oracle does not find vacuous."""
    keys = sorted(census)
    made = [K._row_of(k, census[k]) for k in keys]
    assert _predicted(made) == keys
    pairs = {("GGGATTCGATTTTGAGACGC", 2), ("CCCCGTTGTCAGCATATAGCAGTAAAGGGGACACGGTCATATGTAA", 8)}
    part = {}
    for key, (lv, inputs) in census_all.items():
        mine = [i for i in inputs if (i["pattern"], i["tau"]) in pairs]
        if mine:
            part[key] = (lv, mine)
    assert len(part) > 20
    chosen, left = K.choose_rows(part, oracle)
    assert chosen and set(chosen) | set(left) == set(part)
    rows = [chosen[k] for k in sorted(chosen)]
    assert _predicted(rows) == sorted(chosen)
    for r in rows:
        assert bool(r.knobs) == (part[r.key][0] == 2)
        plan = r.plan()
        text = r.text(plan)
        exp = oracle.buffer_scan(r.pattern, r.tau, text.buf, K.SQ_ALL | (r.options & 0x0C), fasta=r.fasta)
        assert K.vacuity(r, text, exp, plan) is None


def test_batched_planning_equals_planning_one_by_one(harness, rows):
    """harness_plan_many shares one set of automata among the scans of a pattern, as a device pattern does: the same plans as harness_plan,
    which builds them for every call, whatever the order of the scans."""
    H = K.bind(harness)
    for expr, tau in (("GATGTAGCGCGATTAGCCTG", 3), (K.CLASS_PATTERNS[0], 5), ("GATGTAGCGCGATTAGCCTGAAAATGCGAGTACGGCGCGAAT", 15), ("ACGTTGCA", 1)):
        grid, avg = K.census_grid()
        pick = np.arange(0, len(grid), 7)[::-1]          # every seventh scan, knobs first
        many = K.plans_of(H, expr, tau, grid[pick], avg[pick])
        for o, g, a in list(zip(many, grid[pick], avg[pick]))[::5]:
            one = K.plan_of(H, expr, tau, int(g[0]), int(g[1]), float(a), int(g[2]), int(g[3]))
            assert one == dict(zip(K.PLAN_FIELDS, (int(v) for v in o))), (expr, tau, g.tolist(), a)


def test_rows_that_sample_their_text_get_the_plan_of_their_row(rows):
    """The rows that reach their instance through a dirty sample carry no line hint: the context samples the first 64 KiB.  Their text is built
    so that the sample comes out as the row says -- more than one foreign byte in 4 KB, and an average line at which the planner decides as at
    the row's avg_line."""
    sampled = [r for r in rows if r.recipe == "fasta-per-read"]
    assert sampled and all(r.fasta for r in sampled)
    seen = set()
    for r in sampled:
        if (r.pattern, r.tau) in seen:
            continue
        seen.add((r.pattern, r.tau))
        head = r.text().buf[:65536]
        nl = head.count(b"\n")
        foreign = sum(1 for c in head if c not in b"ACGTNacgtn\n")
        assert foreign * 4096 > len(head)                  # seeq_device.hip, scan_setup: sample_dirty
        assert r.plan(avg_line=len(head) / nl) == r.plan()
    for r in rows:
        assert (r.flags != 0) == (r.recipe == "fasta-per-read")

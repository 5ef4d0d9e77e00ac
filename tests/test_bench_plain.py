"""`bench.py` without `--full` does only what its headline needs: set up, warm up, time the steps, write --dump-outputs,
print the line.  The checks, the plain first allocation and the sections run only under `--full`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from conftest import ROOT

SECTIONS = ("end_to_end_pinned_host", "packed_scan", "multi_pattern", "per_call", "fastq_shape", "cpu_baseline", "regions", "cli_wall_clock", "cfg5")


def test_plain_run_plans_nothing_besides_the_steps():
    plan = bench.run_plan(bench.parse_args([]), world=1, rank=0)
    assert not plan["extra"] and plan["first_steps"] == 0 and plan["check_lines"] == 0
    assert plan["candidates"] == 12                     # the allocator's choice of buffer is set-up: it stays
    # the switches of what moved change nothing without --full
    plan = bench.run_plan(bench.parse_args(["--sections", "all", "--first-steps", "5", "--check-lines", "1000"]), world=1, rank=0)
    assert not plan["extra"] and plan["first_steps"] == 0 and plan["check_lines"] == 0


def test_full_run_plans_what_the_default_run_did():
    plan = bench.run_plan(bench.parse_args(["--full"]), world=1, rank=0)
    assert plan["extra"] and plan["first_steps"] == 20 and plan["check_lines"] == 1_000_000 and plan["check_mode"] == "full"
    plan = bench.run_plan(bench.parse_args(["--full", "--gpus", "2"]), world=2, rank=0)
    assert not plan["extra"] and plan["first_steps"] == 0 and plan["check_lines"] == 1_000_000 and plan["check_mode"] == "sample"
    assert plan["candidates"] == 4
    plan = bench.run_plan(bench.parse_args(["--full", "--sections", "none"]), world=1, rank=0)
    assert not plan["extra"] and plan["first_steps"] == 20 and plan["check_mode"] == "full"


@pytest.mark.gpu
def test_plain_line_is_the_headline_alone(gpu, tmp_path):
    """A plain run at a small size: the headline fields, nothing of what moved behind --full, the outputs dumped."""
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--reads", "1500000", "--steps", "3", "--warmup", "1",
                        "--placement-candidates", "3", "--dump-outputs", str(out)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["unit"] == "lines/s" and line["higher_is_better"] is True and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["steps"] == 3 and line["warmup"] == 1 and line["dtype"]
    assert line["results"]["lines"] == 1500000 and line["results"]["oracle_check"] is None
    assert line["placement"]["probed"] == 3 and line["first_allocation"] is None
    assert not [k for k in SECTIONS if k in line], line.keys()
    assert list(line)[-2:] == ["results", "roofline"]
    counts = np.load(out / "counts.npy")
    assert counts[0] == 1500000 and counts[1] == line["results"]["matching_lines"]
    assert len(np.load(out / "records.npy")) == counts[3]

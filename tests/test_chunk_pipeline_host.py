"""The chunk pipeline that drives the three output scans (masp_amd/csrc/chunk_pipeline.h: run_chunks, chunk_outputs) on the CPU: a
stand-alone program, tests/native/chunk_pipeline_host.cpp, runs it over callbacks that only record, built with the address and
undefined-behaviour sanitizers and started as a child process.  The success order is what the scans did before they shared the driver;
the error path (a failing enqueue or collect: a HIP failure, which no GPU test may provoke) is checked here and nowhere else."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "masp_amd", "csrc")
PER = 4
NS_BLOCK, NS_CHUNK_PAIRS = 256, 1 << 18


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chunk_pipeline") / "chunk_pipeline_host")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                           "-I", CSRC, os.path.join(HERE, "native", "chunk_pipeline_host.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and not run.stderr, run.stdout + run.stderr
    return run.stdout.splitlines()


def trace(lines, n, fail):
    """-> rc, [(kind, o0, n, set)] with kind E or C, or ('D', set)"""
    head = "run %d %d %s -> rc " % (n, PER, fail)
    line, = [l for l in lines if l.startswith(head)]
    rc, _, calls = line[len(head):].partition(" :")
    out = []
    for tok in calls.split():
        m = re.fullmatch(r"([EC])(\d+)/(\d+)@([01])", tok)
        out.append((m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))) if m else ("D", int(re.fullmatch(r"D([01])", tok).group(1))))
    return int(rc), out


def chunks_of(n):
    return [(o0, min(PER, n - o0), k & 1) for k, o0 in enumerate(range(0, n, PER))]


@pytest.mark.parametrize("n", [0, 1, PER, PER + 1, 2 * PER, 3 * PER + 1])
def test_success_order(lines, n):
    rc, calls = trace(lines, n, "none")
    assert rc == 0 and not [c for c in calls if c[0] == "D"]
    enq = [c[1:] for c in calls if c[0] == "E"]
    col = [c[1:] for c in calls if c[0] == "C"]
    assert enq == chunks_of(n)                       # the chunks tile [0, n) in order, the sets alternate 0, 1, 0, 1
    assert col == enq                                # every chunk is collected exactly once, the older first (the final ones too)
    for k, c in enumerate(enq):
        assert calls.index(("C",) + c) > calls.index(("E",) + c)
        if k >= 2:                                   # the set's previous chunk: collected right before the set is enqueued again
            assert calls.index(("C",) + enq[k - 2]) == calls.index(("E",) + c) - 1
    tail = calls[calls.index(("E",) + enq[-1]) + 1:] if enq else []
    assert [c[1:] for c in tail] == enq[-2:]         # at most two chunks are in flight at the end
    if n == 3 * PER + 1:
        assert " ".join("%s%d" % c[:2] for c in calls) == "E0 E4 C0 E8 C4 E12 C8 C12"


@pytest.mark.parametrize("kind,code", [("e", 7), ("c", 9)])
@pytest.mark.parametrize("at", range(4))
def test_failure_drains_what_is_in_flight(lines, kind, code, at):
    n = 3 * PER + 1
    rc, calls = trace(lines, n, "%s%d" % (kind, at))
    _, good = trace(lines, n, "none")
    assert rc == code                                # the injected code is the return code
    work = [c for c in calls if c[0] != "D"]
    drains = [c[1] for c in calls if c[0] == "D"]
    assert calls == work + [("D", s) for s in drains]              # no enqueue or collect after the first drain ...
    assert [c for c in work if c[0] == kind.upper()][at] == work[-1]   # ... which follows the failing call at once
    assert work == good[:len(work)]                  # up to the failure: the success order
    failing = work[-1]
    # per set: the last chunk enqueued with success and not collected with success
    pending = {}
    for c in work[:-1]:
        if c[0] == "E":
            pending[c[3]] = c[1:]
        else:
            assert pending.pop(c[3]) == c[1:]
    if failing[0] == "C":
        assert pending.pop(failing[3]) == failing[1:]
    else:
        assert failing[3] not in pending             # (its previous chunk was collected before)
    assert drains[0] == failing[3]                   # the failing set is drained
    assert sorted(drains) == sorted({failing[3]} | set(pending))   # and every set with a chunk pending, each once, no other:
    #                                                  so no set is both collected and drained for the same chunk


def test_chunk_size_rule(lines):
    got = [tuple(int(x) for x in l.split()[1:]) for l in lines if l.startswith("per ")]
    assert [g[0] for g in got] == [1, 32, 1024, 1025, 4096]
    for keys, per, block, pairs in got:
        assert (block, pairs) == (NS_BLOCK, NS_CHUNK_PAIRS)
        assert per == max(NS_BLOCK, NS_CHUNK_PAIRS // keys // NS_BLOCK * NS_BLOCK)
    assert dict((g[0], g[1]) for g in got) == {1: 1 << 18, 32: 8192, 1024: 256, 1025: 256, 4096: 256}   # 4 096 keys: the floor of one workgroup

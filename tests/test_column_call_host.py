"""The body the per-item wallet calls share (masp_amd/csrc/column_call.h: ColumnWidths, column_chunk, ColumnCall, run_columns,
end_columns) on the CPU: a stand-alone program, tests/native/column_call_host.cpp, runs it over plain arrays with a device policy that
records, built with the address and undefined-behaviour sanitizers and started as a child process.  The success order is what
run_nullifiers, run_build_outputs, run_build_spends and run_sign did before they shared the driver; the second chunk of the nullifiers
(2^19 notes a chunk on the GPU) and the error paths (a failing copy, a refused launch: HIP failures, which no GPU test may provoke) are
checked here and nowhere else."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "masp_amd", "csrc")
IN, OUT, STATE = [32, 8, 11, 1, 80], [32, 8, 11, 80, 1], 24   # column widths; the first two inputs are the secret ones where any are
ABSENT_IN, ABSENT_OUT, STATUS = 2, 1, 4
NS = [1, 63, 64, 65, 130]
KINDS = ["M0", "M1", "M2", "M3", "H0", "H3", "Z0", "D0", "D3", "F0"]


def up64(n):
    return (n + 63) // 64 * 64


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("column_call") / "column_call_host")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                           "-I", CSRC, os.path.join(HERE, "native", "column_call_host.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and not run.stderr, run.stdout + run.stderr
    return run.stdout.splitlines()


def case(lines, secrets, n, cap, fail="none"):
    head = "run %d %d %d %s -> " % (secrets, n, cap, fail)
    line, = set(l for l in lines if l.startswith(head))
    facts, work, end, zeros = re.fullmatch(r"(.*?) :(.*?) \|(.*?) \| (.*)", line[len(head):]).groups()
    f = facts.split()
    assert f[0::2][:4] == ["rc", "match", "refused", "rezeroed"] and f[8] == "ms"
    return dict(rc=int(f[1]), match=int(f[3]), refused=int(f[5]), rezeroed=int(f[7]), ms=[float(x) for x in f[9:12]], work=work.split(),
                end=end.split(), zeros=[int(x) for x in zeros.split()])


def chunk_ops(secrets, o, c, n_pad):
    """the operations of the chunk of c items at item o, in the order the four calls had them"""
    ops = ["M0"]
    ops += ["H%d:%d@%s%d" % (k, w * c, "s" if secrets and k < 2 else "", o) for k, w in enumerate(IN) if k != ABSENT_IN]
    ops += ["Z%d" % (sum(OUT[:STATUS]) * n_pad), "M1", "L%d" % c, "M2", "D%d:%d@%d" % (STATUS, c, o)]   # every result but the status bytes
    ops += ["D%d:%d@%d" % (j, w * c, o) for j, w in enumerate(OUT[:STATUS]) if j != ABSENT_OUT]
    return ops + ["M3", "F"]


def all_ops(secrets, n, cap):
    return [op for o in range(0, n, cap) for op in chunk_ops(secrets, o, min(cap, n - o), up64(cap))]


def test_chunk_rule(lines):
    got = [tuple(int(x) for x in re.findall(r"\d+", l)) for l in lines if l.startswith("chunk ")]
    assert sorted(set(g[:3] for g in got)) == sorted((c, d, n) for c in (0, 1, 64, 65) for d in (128, 1 << 16, 1 << 19) for n in NS)
    for configured, default, n, cap, n_pad in got:
        # run_build_outputs' and chunk_cap's expression (the nullifiers' with nothing configured and NF_CHUNK for the default), then n_pad
        assert cap == min(configured if configured else default, (n + 63) // 64 * 64)
        assert n_pad == (cap + 64 - 1) // 64 * 64


def test_layout(lines):
    got = [l.split() for l in lines if l.startswith("layout ")]
    assert sorted(set((int(g[1]), g[2]) for g in got)) == sorted((p, w) for p in (64, 128, 192) for w in ("in", "out", "stage"))
    for g in got:
        n_pad, what, total = int(g[1]), g[2], int(g[3])
        cols = [tuple(int(x) for x in c.split("/")) for c in g[5:]]
        assert [w for _, w in cols] == {"in": IN, "out": OUT, "stage": IN[:2]}[what]
        assert total == sum(w for _, w in cols) * n_pad
        spans = sorted((off, off + w * n_pad) for off, w in cols)
        assert all(off % 64 == 0 for off, _ in spans)
        assert spans[0][0] == 0 and spans[-1][1] <= total
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        assert [off for off, _ in cols] == [sum(w for _, w in cols[:k]) * n_pad for k in range(len(cols))]   # the declared order, no gaps


@pytest.mark.parametrize("secrets", [1, 0])
@pytest.mark.parametrize("n", NS)
def test_chunks_give_the_single_chunk_result_in_the_calls_order(lines, secrets, n):
    caps = sorted({1, 64, 128, up64(n)})
    for cap in caps:
        c = case(lines, secrets, n, cap)
        assert c["rc"] == 0 and c["match"] == 1      # byte for byte what the inputs give: the same for every chunk size
        assert c["refused"] == case(lines, secrets, n, up64(n))["refused"]
        assert c["work"] == all_ops(secrets, n, cap)   # the order; a partial last chunk copies width * c bytes; a chunk's uploads
        #                                                start behind the finish of the chunk before
        chunks = -(-n // cap)
        assert c["ms"] == [0.25 * (k + 1) * chunks * (chunks + 1) / 2 for k in range(3)]   # the sum of (k + 1) (chunk + 1) / 4
        # the ending of a call that succeeded: secrets are scrubbed behind a drained stream, a call without secrets queues nothing
        n_pad = up64(cap)
        assert c["end"] == (["Z%d" % (sum(IN) * n_pad), "Z%d" % (STATE * n_pad), "X"] if secrets else [])
        assert c["zeros"] == ([1, 1, 1] if secrets else [0, 0, -1])
    assert case(lines, secrets, 130, 64)["refused"] > 0
    for cap in (1, 64):                              # a refused item reads zero where the chunk before left an accepted item's bytes
        assert case(lines, secrets, 130, cap)["rezeroed"] > 0


@pytest.mark.parametrize("secrets", [1, 0])
@pytest.mark.parametrize("chunk", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_first_failure_ends_the_call(lines, secrets, chunk, kind):
    n, cap = 130, 64                                 # three chunks
    c = case(lines, secrets, n, cap, "%s@%d" % (kind, chunk))
    good = all_ops(secrets, n, cap)
    per = len(chunk_ops(secrets, 0, cap, cap))
    mine = good[chunk * per:(chunk + 1) * per]
    at = chunk * per + [i for i, op in enumerate(mine) if op[0] == kind[0]][int(kind[1])]
    assert c["rc"] == 40 + chunk                     # the injected code is the return code
    assert c["work"] == good[:at + 1]                # the success order up to the failing operation, and nothing of the driver behind it
    assert c["match"] == 1                           # the chunks finished before it are complete
    assert c["ms"] == [0.25 * (k + 1) * chunk * (chunk + 1) / 2 for k in range(3)]
    # the ending: the stream is drained on every error path, and where the call has secrets they are scrubbed in front of the drain
    assert c["end"] == (["Z%d" % (sum(IN) * cap), "Z%d" % (STATE * cap), "X"] if secrets else ["X"])
    assert c["zeros"] == ([1, 1, 1] if secrets else [0, 0, -1])


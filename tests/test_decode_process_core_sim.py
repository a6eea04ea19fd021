"""CPU: the rules of cmb_decode_process — tests/csrc/decode_process_core_sim.cpp compiled with g++ under AddressSanitizer and
UBSan against cambrian_amd/csrc/decode_process_core.h (the very header decode_process.hip includes) and run directly.  Without
arguments it checks the argument rules and the predicates on hand-made cases; with a table it applies one row's pass in the
kernel's order, and the bits must equal ``processors.apply_torch`` on the same table.

The tables cover: empty and short histories around the n-gram threshold, n-gram size 1, words at n = m - 1 and n = m, repeated
ids, ids without a column (V + 3, -1) in the history and in every list, word offsets out of rule, -inf / +inf / signed zeros,
and random cases with small alphabets."""
import os
import random
import subprocess
import tempfile

import pytest
import torch

from cambrian_amd.model.language_model import processors as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tables():
    """(V, history, spec, logits [V]) per case."""
    inf = float("inf")
    special = torch.tensor([2.5, -2.5, inf, -inf, 0.0, -0.0, 1e-30, -3e38, 7.0])
    out = []
    everything = dict(penalty=1.3, ngram=2, min_new=0, eos=[8, 1], bans=[3], words=[[1, 2], [2, 1, 2], [0, 1, 2, 4]])
    for n in range(0, 8):
        out.append((9, [1, 2, 1, 2, 1, 2, 1][:n], P.ProcessSpec(**everything), special.clone()))
    for g in (1, 2, 3, 4):
        for n in (max(g - 2, 0), g - 1, g, g + 3):
            out.append((9, [5] * n, P.ProcessSpec(ngram=g), special.clone()))
    for m, word in ((2, [4, 6]), (3, [4, 5, 6]), (4, [4, 5, 7, 6])):
        out.append((9, word[:-1], P.ProcessSpec(words=[word]), special.clone()))              # n = m - 1: no ban
        out.append((9, [0] + word[:-1], P.ProcessSpec(words=[word]), special.clone()))        # n = m: ban
    out.append((9, [0, 0, 1, 1, 1, 2, 3, 4, 5, 6, 7, 8, 0], P.ProcessSpec(penalty=0.8), special.clone()))
    out.append((9, [12, 2, 12, -1, 2, 12], P.ProcessSpec(penalty=1.3, ngram=2, min_new=99, eos=[12, 1], bans=[-1, 9, 4],
                                                         words=[[12, 5], [2, 12], [12, 12]]), special.clone()))
    rng = random.Random(11)
    g = torch.Generator().manual_seed(11)
    for _ in range(150):
        V = rng.choice((4, 7, 19))
        a = rng.randint(2, min(V, 5))
        n = rng.randint(0, 30)
        hist = [rng.randrange(a) for _ in range(n)]
        spec = P.ProcessSpec(penalty=rng.choice((1.0, 1.3, 0.8)), ngram=rng.randint(0, 4), min_new=rng.choice((0, 40)),
                             eos=[rng.randrange(V + 2) for _ in range(rng.randint(0, 3))],
                             bans=[rng.randrange(-1, V + 2) for _ in range(rng.randint(0, 2))],
                             words=[[rng.randrange(a) for _ in range(rng.randint(2, 4))] for _ in range(rng.randint(0, 3))])
        spec.penalty = float(torch.tensor(spec.penalty, dtype=torch.float32))
        logits = torch.randn(V, generator=g) * 3
        logits[torch.rand(V, generator=g) < 0.15] = -inf
        out.append((V, hist, spec, logits))
    return out


def _bits(t):
    return [int(v) & 0xFFFFFFFF for v in t.contiguous().view(torch.int32).reshape(-1).tolist()]


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(ROOT, "tests", "csrc", "decode_process_core_sim.cpp")
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "sim")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src,
                        "-o", path], check=True)
        yield path


@pytest.fixture(scope="module")
def sim(exe):
    tables = _tables()
    with tempfile.TemporaryDirectory() as d:
        bare = subprocess.run([exe], capture_output=True, text=True)
        assert bare.returncode == 0 and bare.stdout.strip() == "OK", bare.stdout + bare.stderr
        path = os.path.join(d, "tables.txt")
        with open(path, "w") as f:
            f.write(f"{len(tables)}\n")
            for V, hist, spec, logits in tables:
                eos, bans, ids, off = spec.device_lists("cpu")
                lists = [[] if t is None else t.tolist() for t in (eos, bans, off, ids)]
                pbits = _bits(torch.tensor([spec.penalty], dtype=torch.float32))[0]
                f.write(f"{V} {len(hist)} {spec.ngram} {pbits:x} {spec.min_new} {len(lists[0])} {len(lists[1])} {len(spec.words)} "
                        f"{len(lists[3])}\n")
                for row in lists + [hist]:
                    f.write(" ".join(str(i) for i in row) + "\n")
                f.write(" ".join(f"{b:x}" for b in _bits(logits)) + "\n")
        out = subprocess.run([exe, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.rstrip().endswith("OK"), out.stdout[-2000:]
    rows = {}
    for line in out.stdout.splitlines():
        w = line.split()
        if w[0] == "C":
            rows[int(w[1])] = (int(w[2]), [int(v, 16) for v in w[3:]])
    return tables, rows


def test_core_and_restatement_agree(sim):
    tables, rows = sim
    assert len(rows) == len(tables)
    seen = dict(penalised=0, banned=0, done=0, no_column=0)
    for c, (V, hist, spec, logits) in enumerate(tables):
        n = len(hist)
        h = torch.tensor([hist + [0]], dtype=torch.int64)              # one spare column: n = 0 needs a row to slice
        done = torch.zeros(1, dtype=torch.bool)
        want = P.apply_torch(logits.clone()[None], h, n, spec, done)[0]
        got_done, got = rows[c]
        assert got == _bits(want), (c, V, hist, spec)
        assert got_done == int(done[0]), (c, hist, spec.eos)
        fin = torch.isfinite(logits)
        seen["penalised"] += int(bool((want[fin] != logits[fin]).logical_and(torch.isfinite(want[fin])).any()))
        seen["banned"] += int(bool((want[fin] == float("-inf")).any()))
        seen["done"] += got_done
        seen["no_column"] += int(any(not 0 <= i < V for i in hist + spec.eos + spec.bans))
    assert all(v >= 10 for v in seen.values()), seen


def test_word_offsets_out_of_rule_ban_nothing(exe):
    """The table format lets the offsets lie; the simulator must neither ban nor read outside its exact-size arrays."""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "t.txt")
        zeros = " ".join(["0"] * 6)
        with open(path, "w") as f:
            # 3 "words" over 4 ids: offsets 0 2 | 2 9 (past the ids) | 9 1 (backwards); history 1 3
            f.write(f"1\n6 2 0 3f800000 0 0 0 3 4\n\n\n0 2 9 1\n3 4 3 5\n1 3\n{zeros}\n")
        out = subprocess.run([exe, path], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("OK"), out.stdout + out.stderr
    row = [l for l in out.stdout.splitlines() if l.startswith("C ")][0].split()[3:]
    assert [int(v, 16) for v in row] == [0, 0, 0, 0, 0xFF800000, 0]       # only the well-formed word (3, 4) after "... 3" bans 4

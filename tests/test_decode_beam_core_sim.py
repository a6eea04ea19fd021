"""CPU: the bookkeeping of cmb_decode_beam — tests/csrc/decode_beam_core_sim.cpp compiled with g++ under AddressSanitizer and
UBSan against cambrian_amd/csrc/decode_beam_core.h (the very header decode_beam.hip includes) and run directly on small
synthetic log-probability tables; the same tables go through the torch restatement (model/language_model/beam.py) and every
step's parents, tokens, scores (bit for bit), hypotheses, flags and sequences must agree.

The tables cover: equal scores everywhere (the order is the flat index), the first step seeing beam 0 only, the last step
finishing every top candidate, hypotheses displaced in the merge, the sticky flag, and steps run on after the stop."""
import os
import struct
import subprocess
import tempfile

import pytest
import torch

from cambrian_amd.model.language_model import beam as BM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x: float) -> int:
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _tables():
    """(name, nb, V, steps, max_new, eos, logits [steps, nb, V]); the simulator is fed log_softmax(logits)."""
    out = []
    gen = torch.Generator().manual_seed(17)
    out.append(("all_equal", 3, 7, 4, 4, None, torch.zeros(4, 3, 7)))
    out.append(("identical_rows", 4, 5, 5, 5, 2, (torch.randn(5, 1, 5, generator=gen) * 2).round().expand(5, 4, 5).clone()))
    quant = (torch.randn(6, 2, 9, generator=gen) * 2).round() / 2
    out.append(("quantised", 2, 9, 6, 6, 4, quant))
    for seed, nb, V, eos in ((1, 2, 6, 0), (2, 3, 6, 1), (3, 4, 8, 2), (4, 8, 5, 3), (5, 16, 3, 1), (6, 3, 2, 0), (7, 2, 11, None)):
        g = torch.Generator().manual_seed(100 + seed)
        steps = 10
        logits = torch.randn(steps, nb, V, generator=g) * 1.5
        if eos is not None:
            logits[:, :, eos] += 1.5                       # a frequent eos: hypotheses finish early and displace each other
        out.append((f"random{seed}", nb, V, steps, steps, eos, logits))
    # the search stops long before max_new; the steps after the stop are run all the same
    g = torch.Generator().manual_seed(9)
    logits = torch.randn(12, 2, 6, generator=g)
    logits[:, :, 3] += 6.0
    out.append(("runs_on", 2, 6, 12, 40, 3, logits))
    return out


@pytest.fixture(scope="module")
def sim():
    src = os.path.join(ROOT, "tests", "csrc", "decode_beam_core_sim.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "sim")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src,
                        "-o", exe], check=True)
        tables = _tables()
        path = os.path.join(d, "tables.txt")
        with open(path, "w") as f:
            f.write(f"{len(tables)}\n")
            for _, nb, V, steps, max_new, eos, logits in tables:
                f.write(f"{nb} {V} {steps} {max_new} {-1 if eos is None else eos}\n")
                lp = torch.log_softmax(logits.float(), dim=-1)
                for s in range(steps):
                    f.write(" ".join(f"{_bits(float(v)):x}" for v in lp[s].reshape(-1)) + "\n")
        bare = subprocess.run([exe], capture_output=True, text=True)
        assert bare.returncode == 0 and "OK" in bare.stdout, bare.stdout + bare.stderr
        out = subprocess.run([exe, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.rstrip().endswith("OK"), out.stdout[-2000:]
    trace = {}
    cur = None
    for line in out.stdout.splitlines():
        w = line.split()
        if w[0] == "S":
            parts = [p.split() for p in line.split("|")]
            cur = trace.setdefault((int(w[1]), int(w[2])), {"R": {}, "F": {}})
            cur.update(parent=[int(v) for v in parts[1]], tok=[int(v) for v in parts[2]], run_score=[int(v, 16) for v in parts[3]],
                       fin_score=[int(v, 16) for v in parts[4]], fin_len=[int(v) for v in parts[5]],
                       fin_ok=[int(v) for v in parts[6]], unsat=int(parts[7][0]), all_hit=int(parts[7][1]))
        elif w[0] in "RF":
            cur[w[0]][int(w[1])] = [int(v) for v in w[2:]]
    return tables, trace


def _f32_bits(t: torch.Tensor):
    return [int(v) & 0xFFFFFFFF for v in t.contiguous().view(torch.int32).tolist()]


def test_core_and_restatement_agree_step_by_step(sim):
    tables, trace = sim
    seen = dict(displaced=0, flag_fell=0, ran_on=0, early_done=0)
    for cs, (name, nb, V, steps, max_new, eos, logits) in enumerate(tables):
        st = BM.BeamState(1, nb, max_new)
        done_at = None
        for s in range(steps):
            before_score, before_ok, before_len = st.fin_score.clone(), st.fin_ok.clone(), st.fin_len.clone()
            was_unsat = bool(st.unsat[0])
            parent, tok = BM.beam_update(st, logits[s], s, eos, s + 1 == max_new)
            got = trace[(cs, s)]
            what = (name, s)
            assert got["parent"] == parent[0].tolist() and got["tok"] == tok[0].tolist(), what
            assert got["run_score"] == _f32_bits(st.run_score[0]), what
            assert got["fin_score"] == _f32_bits(st.fin_score[0]), what
            assert got["fin_len"] == st.fin_len[0].tolist() and got["fin_ok"] == st.fin_ok[0].long().tolist(), what
            assert got["unsat"] == int(st.unsat[0]) and got["all_hit"] == int(st.all_hit[0]), what
            for i in range(nb):
                assert got["R"][i] == st.run_ids[0, i, :s + 1].tolist(), what
                assert got["F"][i] == st.fin_ids[0, i, :int(st.fin_len[0, i])].tolist(), what
            if s == 0 and V > nb:                             # a shorter row cannot fill the beams by itself
                assert got["parent"] == [0] * nb, "the first step sees beam 0 only"
            if s + 1 == max_new:
                assert all(got["fin_ok"]) and got["all_hit"] == 1, "the last step finishes every top candidate"
            # an earlier finished hypothesis moved down or out
            if bool(before_ok.any()) and not torch.equal(before_score[0][before_ok[0]], st.fin_score[0][:int(before_ok.sum())]):
                seen["displaced"] += 1
            if was_unsat and not bool(st.unsat[0]):
                seen["flag_fell"] += 1
            if done_at is not None:                           # after the stop nothing about the hypotheses changes
                assert not bool(st.unsat[0]), (what, "the flag is sticky")
                assert torch.equal(st.fin_score, before_score) and torch.equal(st.fin_ok, before_ok), what
                assert torch.equal(st.fin_len, before_len), what
                seen["ran_on"] += 1
            elif BM.beam_done(st) and s + 1 < max_new:
                done_at = s
                seen["early_done"] += 1
        if name == "all_equal":
            assert trace[(cs, 1)]["tok"] == [0, 1, 2] and trace[(cs, 1)]["parent"] == [0, 0, 0]
    print(seen)
    assert all(seen.values()), seen

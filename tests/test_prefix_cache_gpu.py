"""`-m gpu`: the reusable prompt prefix — ``prefill_prefix`` / ``generate(suffix_ids, prefix=cache)`` and ``extend_step`` on top of
``ops.extend_attention``.  The contract: row n of a prefix call returns what ``generate(cat(prefix_ids, suffix_n), images=...)``
returns for that prompt alone.  fp32 models compare tokens; bf16 models compare the first step's logits through ``rel_err``
(``TOL["bf16"]``; with images the two bounds of test_dynamic_gpu.py::test_dynamic_end_to_end_logits_match_oracle)."""
import pytest
import torch

from conftest import TOL, rel_err
from test_decode_step_gpu import _lm
from test_dynamic_gpu import _eval_batch
from test_model_gpu import _build, P0

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SWITCHES = ("CAMBRIAN_AMD_DECODE_STEP", "CAMBRIAN_AMD_DECODE_FP8", "CAMBRIAN_AMD_DECODE_FP4", "CAMBRIAN_AMD_DECODE_LINEAR",
            "CAMBRIAN_AMD_DECODE_ATTN", "CAMBRIAN_AMD_DECODE_KV_FP8", "CAMBRIAN_AMD_DECODE_SAMPLE", "CAMBRIAN_AMD_DECODE_PROCESS")


def _CL():
    from cambrian_amd.model.language_model import cambrian_llama as CL
    return CL


@pytest.fixture()
def clean_env(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def _ids(dev, n, seed):
    return torch.randint(1, 64, (1, n), generator=torch.Generator().manual_seed(seed)).to(dev)


def _first_logits(model, cache, suffix, mask=None):
    """fp32 logits [N, V] of the prefix path's first step: ``extend_step`` over the suffixes + lm_head (``_prefix_extend``)."""
    with torch.no_grad():
        return _CL()._prefix_extend(model, cache, suffix, mask, 0)[0]


def _left_padded(suffixes, dev):
    """N suffixes [1, q_n] -> (ids [N, Q], mask [N, Q]) left-padded to the longest."""
    Q = max(s.shape[1] for s in suffixes)
    ids = torch.zeros(len(suffixes), Q, dtype=torch.int64, device=dev)
    mask = torch.zeros(len(suffixes), Q, dtype=torch.bool, device=dev)
    for n, s in enumerate(suffixes):
        ids[n, Q - s.shape[1]:] = s[0]
        mask[n, Q - s.shape[1]:] = True
    return ids, mask


# ---------------------------------------------------------------------------------------------------------------------
# text-only model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lm", ["llama", "phi3"])
def test_fp32_tokens_equal_the_whole_prompt_call(dev, clean_env, lm):
    model = _lm(dev, lm, torch.float32)
    for P in (9, 130):
        head = _ids(dev, P, P)
        cache = model.prefill_prefix(head)
        assert cache.P == P and cache.n_tok == P and len(cache.kv) == len(model.model.layers)
        for Q in (1, 5, 40):
            tail = _ids(dev, Q, 100 * P + Q)
            want = model.generate(torch.cat([head, tail], 1), max_new_tokens=4)
            got = model.generate(tail, prefix=cache, max_new_tokens=4)
            assert torch.equal(got, want), f"{lm} P={P} Q={Q}: {got.tolist()} vs {want.tolist()}"


@pytest.mark.parametrize("lm", ["llama", "phi3"])
def test_bf16_first_step_logits(dev, clean_env, lm, monkeypatch):
    from cambrian_amd import ops
    model = _lm(dev, lm, BF)
    calls = []
    real = ops.extend_attention
    monkeypatch.setattr(ops, "extend_attention", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    for P in (9, 130):
        head = _ids(dev, P, P)
        cache = model.prefill_prefix(head)
        for Q in (1, 5, 40):
            tail = _ids(dev, Q, 100 * P + Q)
            with torch.no_grad():
                want = model(input_ids=torch.cat([head, tail], 1)).logits[:, -1]
            del calls[:]
            got = _first_logits(model, cache, tail)
            assert len(calls) == len(model.model.layers)               # the kernel, not the torch body
            e = rel_err(got, want)
            print(f"{lm} P={P} Q={Q}: first-step logits rel err {e:.3g}")
            assert e < TOL["bf16"], f"{lm} P={P} Q={Q}: {e}"


@pytest.mark.parametrize("name,dt", [("fp32", torch.float32), ("bf16", BF)])
def test_batched_left_padded_suffixes(dev, clean_env, name, dt):
    model = _lm(dev, "llama", dt)
    head = _ids(dev, 37, 1)
    cache = model.prefill_prefix(head)
    tails = [_ids(dev, q, 50 + q) for q in (3, 20, 11)]
    ids, mask = _left_padded(tails, dev)
    if dt == torch.float32:
        got = model.generate(ids, prefix=cache, attention_mask=mask, max_new_tokens=4)
        for n, t in enumerate(tails):
            one = model.generate(t, prefix=cache, max_new_tokens=4)
            whole = model.generate(torch.cat([head, t], 1), max_new_tokens=4)
            assert torch.equal(got[n:n + 1], one) and torch.equal(one, whole), f"row {n}"
    else:
        got = _first_logits(model, cache, ids, mask)
        for n, t in enumerate(tails):
            e = rel_err(got[n:n + 1], _first_logits(model, cache, t))
            print(f"row {n}: batched against single, logits rel err {e:.3g}")
            assert e < TOL["bf16"], f"row {n}: {e}"


def test_a_prefix_cache_serves_many_calls_and_is_never_written(dev, clean_env):
    model = _lm(dev, "llama", BF)
    cache = model.prefill_prefix(_ids(dev, 37, 1))
    before = [(k.clone(), v.clone()) for k, v in cache.kv], cache.key_mask.clone(), cache.last_hidden.clone()
    a, b = _ids(dev, 7, 2), _ids(dev, 19, 3)
    first = model.generate(a, prefix=cache, max_new_tokens=4)
    model.generate(b, prefix=cache, max_new_tokens=4)
    third = model.generate(a, prefix=cache, max_new_tokens=4)
    assert torch.equal(first, third)
    for (k0, v0), (k, v) in zip(before[0], cache.kv):
        assert torch.equal(k0.view(torch.int16), k.view(torch.int16)) and torch.equal(v0.view(torch.int16), v.view(torch.int16))
    assert torch.equal(before[1], cache.key_mask) and torch.equal(before[2].view(torch.int16), cache.last_hidden.view(torch.int16))


@pytest.mark.parametrize("switch", ["CAMBRIAN_AMD_DECODE_STEP", "CAMBRIAN_AMD_DECODE_FP8"])
def test_the_decode_switches_still_compose(dev, clean_env, switch):
    """bf16 model under the one-call step / the e4m3 weight stream: the prefix call returns the tokens of the whole-prompt call
    under the same switch, and the switched kernel runs.  All four tokens are compared, for both switches: neither diverges on
    this model (no near-tie among its first four steps)."""
    from cambrian_amd import ops
    clean_env.setenv(switch, "1")
    name = "decode_step" if switch.endswith("STEP") else "decode_linear_fp8"
    calls, real = [], getattr(ops, name)
    clean_env.setattr(ops, name, lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    model = _lm(dev, "llama", BF)
    head, tail = _ids(dev, 37, 1), _ids(dev, 9, 2)
    cache = model.prefill_prefix(head)
    want = model.generate(torch.cat([head, tail], 1), max_new_tokens=4)
    del calls[:]
    got = model.generate(tail, prefix=cache, max_new_tokens=4)
    assert calls, f"{switch}=1: {name} did not run under generate(prefix=...)"
    print(f"{switch}: prefix call {got.tolist()}, whole prompt {want.tolist()}")
    assert got.shape == (1, 4) and torch.equal(got, want)


# ---------------------------------------------------------------------------------------------------------------------
# with images and the in-LLM SVA hook
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dt,tol", [("fp32", torch.float32, 1e-3), ("bf16", BF, 5e-2)])
def test_image_prefix(dev, clean_env, name, dt, tol):
    from cambrian_amd import ops
    monkeypatch = clean_env
    model, cfg, towers = _build(dev, dt, monkeypatch)
    model.eval()
    ids, att, sizes, images = _eval_batch(dev, dt, towers)
    ids, sizes, images = ids[:1].to(dev), sizes[1:2], [i[1:2].to(dev, dt) for i in images]     # one wide image, no padding
    cut = P0 + 3                                                        # through the image token plus two more
    head, tail = ids[:, :cut], ids[:, cut:]
    want = model.generate(ids, images=images, image_sizes=sizes, max_new_tokens=4)
    model._dynamic_path = True
    with torch.no_grad():
        want_logits = model(input_ids=ids, images=images, image_sizes=sizes).logits[:, -1]
    model._dynamic_path = False
    cache = model.prefill_prefix(head, images=images, image_sizes=sizes)
    assert cache.P > cut                                                # the length after the image expansion

    counts = {"tower": 0, "prepare": 0, "extend": 0}

    def spy(key, real):
        def f(*a, **kw):
            counts[key] += 1
            return real(*a, **kw)
        return f

    for t in towers:
        monkeypatch.setattr(t, "forward", spy("tower", t.forward))
    monkeypatch.setattr(model, "prepare_inputs_labels_for_multimodal", spy("prepare", model.prepare_inputs_labels_for_multimodal))
    monkeypatch.setattr(ops, "extend_attention", spy("extend", ops.extend_attention))
    got = model.generate(tail, prefix=cache, max_new_tokens=4)
    assert counts["tower"] == 0 and counts["prepare"] == 0
    assert counts["extend"] == (len(model.model.layers) if dt == BF else 0)
    e = rel_err(_first_logits(model, cache, tail), want_logits)
    print(f"{name}: last-position logits rel err {e:.3g}; prefix call {got.tolist()}, whole prompt {want.tolist()}")
    assert e < tol, f"{name}: last-position logits rel err {e}"
    if dt == torch.float32:
        assert torch.equal(got, want)

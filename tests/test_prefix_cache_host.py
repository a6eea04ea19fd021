"""CPU: what ``generate(prefix=...)`` refuses, each with a CPU model whose every entry point into the decoder raises — the
checks run before the model is touched.  The ``PrefixCache`` is built by hand (``prefill_prefix`` itself needs the GPU)."""
import pytest
import torch

from test_decode_step_gpu import _lm

P, NKV, HD, LAYERS = 6, 2, 64, 2


def _cache(CL, model, dtype=torch.float32, device=torch.device("cpu"), layers=LAYERS):
    kv = [(torch.zeros(1, NKV, P, HD, dtype=dtype), torch.zeros(1, NKV, P, HD, dtype=dtype)) for _ in range(layers)]
    return CL.PrefixCache(model, kv, torch.ones(1, P, dtype=torch.bool), P, torch.zeros(1, 256, dtype=dtype), dtype, device)


@pytest.fixture()
def setup(monkeypatch):
    from cambrian_amd import ops
    from cambrian_amd.model.language_model import cambrian_llama as CL
    for name in ("CAMBRIAN_AMD_DECODE_KV_FP8", "CAMBRIAN_AMD_DECODE_BEAM"):
        monkeypatch.delenv(name, raising=False)
    model = _lm("cpu", "llama", torch.float32)

    def touched(*a, **kw):
        raise AssertionError("the model was touched before the refusal")

    for mod in (model.model, model.lm_head, model.model.embed_tokens):
        monkeypatch.setattr(mod, "forward", touched)
    for name in ("extend_step", "_prefix_extend", "_prefill", "_bf16_prefill"):
        monkeypatch.setattr(CL, name, touched)
    for name in ("extend_attention", "rope_table", "rope"):
        monkeypatch.setattr(ops, name, touched)
    return CL, model, _cache(CL, model)


def test_prefix_is_a_known_argument_and_the_checks_pass_a_legal_call(setup):
    """A legal call gets through every refusal and reaches the model (which this fixture makes raise): ``prefix`` is not an
    unknown argument."""
    CL, model, cache = setup
    ids = torch.tensor([[0, 5, 7], [3, 4, 9]])
    mask = torch.tensor([[0, 1, 1], [1, 1, 1]])
    with pytest.raises(AssertionError, match="the model was touched"):
        model.generate(ids, prefix=cache, attention_mask=mask, max_new_tokens=2)
    with pytest.raises(AssertionError, match="the model was touched"):
        model.generate(ids, prefix=cache, max_new_tokens=2, prompt_lookup_num_tokens=0, num_beams=1)


def test_value_errors(setup):
    CL, model, cache = setup
    from cambrian_amd.constants import IMAGE_TOKEN_INDEX
    ids = torch.tensor([[2, 5, 7], [3, 4, 9]])
    for mask in ([[1, 1, 0], [1, 1, 1]], [[1, 0, 1], [1, 1, 1]], [[0, 0, 0], [1, 1, 1]], [[1, 1, 1]]):
        with pytest.raises(ValueError, match="left-padded"):
            model.generate(ids, prefix=cache, attention_mask=torch.tensor(mask))
    with pytest.raises(ValueError, match="Q >= 1"):
        model.generate(torch.zeros(2, 0, dtype=torch.int64), prefix=cache)
    with pytest.raises(ValueError, match="image token"):
        model.generate(torch.tensor([[2, IMAGE_TOKEN_INDEX, 7]]), prefix=cache)
    with pytest.raises(ValueError, match="images belong to the prefix"):
        model.generate(ids, prefix=cache, images=[torch.zeros(1, 3, 8, 8)])
    with pytest.raises(ValueError, match="image sizes belong to the prefix"):
        model.generate(ids, prefix=cache, image_sizes=[(8, 8)])
    with pytest.raises(ValueError, match="position ids are not taken"):
        model.generate(ids, prefix=cache, position_ids=torch.arange(3)[None].expand(2, 3))
    with pytest.raises(ValueError, match="PrefixCache"):
        model.generate(ids, prefix=[(torch.zeros(1), torch.zeros(1))])
    other = _lm("cpu", "llama", torch.float32)
    for wrong in (_cache(CL, other), _cache(CL, model, dtype=torch.bfloat16), _cache(CL, model, device=torch.device("meta")),
                  _cache(CL, model, layers=1)):
        with pytest.raises(ValueError, match="another model"):
            model.generate(ids, prefix=wrong)


def test_not_implemented(setup, monkeypatch):
    CL, model, cache = setup
    ids = torch.tensor([[2, 5, 7]])
    with pytest.raises(NotImplementedError, match="num_beams"):
        model.generate(ids, prefix=cache, num_beams=3)
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_BEAM", "1")              # switched on for whole prompts; still not on a prefix
    with pytest.raises(NotImplementedError, match="cached prefix"):
        model.generate(ids, prefix=cache, num_beams=3)
    with pytest.raises(NotImplementedError, match="prompt-lookup"):
        model.generate(ids, prefix=cache, prompt_lookup_num_tokens=4)
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_KV_FP8", "1")
    with pytest.raises(NotImplementedError, match="CAMBRIAN_AMD_DECODE_KV_FP8"):
        model.generate(ids, prefix=cache)
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_KV_FP8")
    model.config.decode_kv_fp8 = True
    with pytest.raises(NotImplementedError, match="config.decode_kv_fp8"):
        model.generate(ids, prefix=cache)

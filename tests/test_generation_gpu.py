"""KV-cache generation on the GPU (bf16 kernels) against an fp32 copy of the same
weights: teacher-forced decode logits, and greedy / ragged generation checked for
consistency with the existing full forward."""
import pytest
import torch

from test_generation_cpu import MODELS, make_model

pytestmark = pytest.mark.gpu

dev = "cuda"


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


_pairs = {}


def model_pair(kind):
    """(bf16 model, fp32 copy of the same weights), both on the GPU; shared, unchanged."""
    if kind not in _pairs:
        m = make_model(kind, dev, "bfloat16")
        ref = make_model(kind, dev, "float32")
        ref.load_state_dict({k: v.float() for k, v in m.state_dict().items()})
        _pairs[kind] = (m, ref)
    return _pairs[kind]


@pytest.mark.parametrize("kind", MODELS)
def test_teacher_forced_logits(kind):
    """Prefill 8 tokens, feed tokens 8..23 one at a time through decode_step; the logits
    at positions 7..22 must be at most twice as far from the fp32 copy as the bf16 full
    forward's (E_full)."""
    model, ref = model_pair(kind)
    torch.manual_seed(3)
    B, S, P = 2, 24, 8
    ids = torch.randint(1, model.cfg.vocab_size, (B, S), device=dev)
    with torch.no_grad():
        want = ref(ids)[:, P - 1:S - 1].float()
        full = model(ids)[:, P - 1:S - 1].float()
        cache = model.init_cache(B, S)
        got = [model.prefill(ids[:, :P], cache)]
        for t in range(P, S):
            got.append(model.decode_step(ids[:, t], cache))
    assert cache.lens.tolist() == [S, S]
    dec = torch.stack(got[:-1], 1).float()  # positions 7..22 (the last step predicts position 24)
    e_full, e_dec = _rel(full, want), _rel(dec, want)
    print(f"teacher-forced {kind}: E_full {e_full:.3e}  E_decode {e_dec:.3e}")
    assert torch.isfinite(dec).all()
    assert e_dec <= 2 * e_full


def _check_consistent(model, ref, seq, new, first, what):
    """Every emitted token's full-forward logit is within 2 * A_full of its row maximum
    (A_full: largest |bf16 full-forward logit - fp32 copy's logit| on this sequence)."""
    with torch.no_grad():
        full = model(seq).float()
        a_full = (full - ref(seq).float()).abs().max().item()
    worst = 0.0
    for b in range(seq.shape[0]):
        for i in range(new.shape[1]):
            row = full[b, first[b] + i - 1]  # the position that predicts emitted token i
            worst = max(worst, (row.max() - row[new[b, i]]).item())
    print(f"{what}: A_full {a_full:.3e}  worst gap of an emitted token {worst:.3e}")
    assert worst <= 2 * a_full


@pytest.mark.parametrize("kind", MODELS)
def test_greedy_consistent_with_full_forward(kind):
    model, ref = model_pair(kind)
    torch.manual_seed(4)
    ids = torch.randint(1, model.cfg.vocab_size, (2, 5), device=dev)
    toks, lengths = model.generate(ids, 8)
    assert toks.shape == (2, 8) and lengths.tolist() == [8, 8]
    _check_consistent(model, ref, torch.cat([ids, toks], 1), toks, [5, 5], f"greedy {kind}")


@pytest.mark.parametrize("kind", MODELS)
def test_ragged_prompts_gpu(kind):
    model, ref = model_pair(kind)
    torch.manual_seed(5)
    rows = [torch.randint(1, model.cfg.vocab_size, (n,), device=dev) for n in (3, 7)]
    padded = torch.zeros(2, 7, dtype=torch.long, device=dev)
    for b, r in enumerate(rows):
        padded[b, : len(r)] = r
    toks, _ = model.generate(padded, 8, prompt_lens=[3, 7])
    for b, r in enumerate(rows):
        seq = torch.cat([r, toks[b]])[None]
        _check_consistent(model, ref, seq, toks[b: b + 1], [len(r)], f"ragged {kind} row {b}")

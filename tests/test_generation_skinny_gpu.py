"""KV-cache generation with the decode-step GEMMs on the skinny-M kernels
(``FLAGS_skinny_gemm``, ops/skinny.py): logit accuracy against an fp32 copy of the weights,
the number of skinny launches per step with the flag on and off, and run-to-run bits.
B = 1 and 3 are batch sizes whose GEMMs ran on vendor code before."""
import pytest
import torch

from paddle_amd.ops import skinny
from paddle_amd.utils import flags
from test_generation_cpu import MODELS, make_model

pytestmark = pytest.mark.gpu

dev = "cuda"
BATCHES = [1, 3, 8]


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


class skinny_flag:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.prev = flags.get("skinny_gemm")
        flags.set("skinny_gemm", self.on)

    def __exit__(self, *exc):
        flags.set("skinny_gemm", self.prev)


class count_launches:
    def __enter__(self):
        self.n = 0
        self._orig = skinny._launch

        def wrapped(*a, **k):
            self.n += 1
            return self._orig(*a, **k)

        skinny._launch = wrapped
        return self

    def __exit__(self, *exc):
        skinny._launch = self._orig


def _teacher_forced(model, ids, P):
    """Prefill P tokens, then feed the rest one at a time; logits of positions P-1 .. S-2 and
    the skinny launches of the prefill and of each decode step."""
    B, S = ids.shape
    cache = model.init_cache(B, S)
    with count_launches() as c:
        got = [model.prefill(ids[:, :P], cache)]
    n_prefill, n_steps = c.n, []
    for t in range(P, S):
        with count_launches() as c:
            got.append(model.decode_step(ids[:, t], cache))
        n_steps.append(c.n)
    assert cache.lens.tolist() == [S] * B
    return torch.stack(got[:-1], 1).float(), n_prefill, n_steps


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("kind", MODELS)
@pytest.mark.parametrize("on", [True, False])
def test_teacher_forced_logits_and_launch_counts(kind, B, on):
    """E_decode <= 2 * E_full against the fp32 copy with the flag on and off; on: 4 skinny
    launches per layer + the head per decode step (9 for the two-layer models) and 1 in the
    prefill (its last-row logits); off: none."""
    model, ref = model_pair(kind)
    torch.manual_seed(3)
    S, P = 24, 8
    ids = torch.randint(1, model.cfg.vocab_size, (B, S), device=dev)
    with torch.no_grad():
        want = ref(ids)[:, P - 1:S - 1].float()
        full = model(ids)[:, P - 1:S - 1].float()
    with skinny_flag(on):
        dec, n_prefill, n_steps = _teacher_forced(model, ids, P)
    e_full, e_dec = _rel(full, want), _rel(dec, want)
    print(f"teacher-forced {kind} B={B} skinny={'on' if on else 'off'}: E_full {e_full:.3e}  E_decode {e_dec:.3e}  "
          f"launches prefill {n_prefill} step {n_steps[0]}")
    assert torch.isfinite(dec).all()
    assert e_dec <= 2 * e_full
    layers = model.cfg.num_hidden_layers
    assert n_prefill == (1 if on else 0)
    assert n_steps == [(4 * layers + 1) if on else 0] * (S - P)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("kind", MODELS)
def test_run_to_run_bits(kind, B):
    model, _ = model_pair(kind)
    torch.manual_seed(11)
    ids = torch.randint(1, model.cfg.vocab_size, (B, 6), device=dev)
    with skinny_flag(True):
        a, _ = model.generate(ids, 8)
        b, _ = model.generate(ids, 8)
        assert torch.equal(a, b)
        runs = []
        for _ in range(2):
            cache = model.init_cache(B, 12)
            logits = [model.prefill(ids, cache)]
            for t in range(4):
                logits.append(model.decode_step(a[:, t], cache))
            runs.append(torch.stack(logits))
        assert torch.equal(runs[0], runs[1])

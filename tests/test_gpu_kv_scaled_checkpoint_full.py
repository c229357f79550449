"""The per-row scaled fp8 KV cache on the written full-size checkpoint of
tests/test_gpu_checkpoint_full.py (Llama-3.2-1B geometry, trained-like
weights whose V rows sit largely in or under e4m3's subnormal band at unit
scale): the same 768-row decode step with an fp8 and an fp8s cache in one
run, each against the fp32 reference rows.

Asserted: fp8s's logit cosine is not below fp8's by more than 0.001, the
spread between the two fp8 values recorded in profiles/checkpoint_full_r6.txt
(0.991-0.992).  No absolute target: none has been measured.  Both numbers are
printed (recorded in profiles/checkpoint_full_kv_scaled.txt and
docs/KERNELS.md)."""
import pytest
import torch

from tests.test_gpu_checkpoint_full import V, _cos, _load, _prompts, ckpt  # noqa: F401

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

SPREAD = 0.001


def _decode_768(ckpt, kv):  # noqa: F811
    """The step of test_full_checkpoint_768_row_decode_on_the_default_kernels
    (same seeds, prompts, rows); cosines of rows 0, 3, 7 against fp32."""
    m = _load(ckpt, max_batch=512, max_rows=768, max_seq=512, kv_dtype=kv)
    assert m.use_tgemm and m.tg_head and m.kv_scaled == (kv == "fp8s")
    g = torch.Generator().manual_seed(2)
    base = _prompts(1, g)[0][:60]
    n_slots, rows = 512, 768
    prompts = [base[:30] + _prompts(1, g)[0][1:31] for _ in range(8)]
    for b in range(0, n_slots, 64):
        m.prefill_batch([(prompts[s % 8], s, 0) for s in range(b, b + 64)])
    nxt = [int(t) for t in torch.randint(0, V - 256, (8,), generator=g)]
    tk = torch.tensor([nxt[r % 8] if r < n_slots else nxt[(r - n_slots) % 8] for r in range(rows)],
                      dtype=torch.int32, device="cuda")
    sl = torch.tensor([r % n_slots for r in range(rows)], dtype=torch.int32, device="cuda")
    ps = torch.tensor([60 + (r // n_slots) for r in range(rows)], dtype=torch.int32, device="cuda")
    tk[n_slots:] = tk[:rows - n_slots]
    logits = m.decode(tk, sl, ps).float()
    coss = [_cos(logits[r], m.reference_logits(prompts[r % 8] + [nxt[r % 8]])[-1].float()) for r in (0, 3, 7)]
    del m
    torch.cuda.empty_cache()
    return coss


def test_full_checkpoint_768_row_decode_fp8s_against_fp8(ckpt):  # noqa: F811
    cos = {kv: _decode_768(ckpt, kv) for kv in ("fp8", "fp8s")}
    for kv, c in cos.items():
        print(f"768-row decode ({kv} KV) logit cosine", [round(x, 5) for x in c])
    assert min(cos["fp8s"]) >= min(cos["fp8"]) - SPREAD, cos

"""A tiny Qwen2-layout checkpoint whose K bias takes post-RoPE K rows past
e4m3's +-448, and its last-position logits through the engine's step sizes
with each KV-cache format (shared by the CPU and the GPU fp8s tests)."""
import torch

from dmcp.models.llm import LocalLM
from dmcp.utils import synth

VOCAB = 512


def biased_checkpoint(root: str, k_bias_scale: float = 400.0, head_dim: int = 64) -> str:
    return synth.llama_checkpoint(root, layers=2, hidden=256, heads=4, kv_heads=2, intermediate=512, vocab=VOCAB,
                                  tokenizer="", outliers=(7,), seed=5, device="cpu", qkv_bias=True,
                                  model_type="qwen2", head_dim=head_dim, k_bias_scale=k_bias_scale)


def _tokens(n: int, seed: int) -> list:
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, VOCAB, (n,), generator=g).tolist()


def max_k(ckpt: str) -> float:
    """The largest |K| the bf16-cache CPU model caches for the test prompt."""
    m = LocalLM.load_safetensors(ckpt, device="cpu", max_batch=2, max_rows=2, max_seq=64, kv_dtype="bf16")
    m.forward_tokens(torch.tensor(_tokens(40, 1), dtype=torch.int32), 0, 0)
    return float(m.k_cache.float().abs().max())


def step_errors(ckpt: str, kv: str, device: str, rows=(16,), prompt: int = 40, against: str = "fp32") -> dict:
    """max |logit - fp32 reference| / max |reference logit| of the last
    position after a prefill of ``prompt`` tokens, and over every row of one
    decode step of each of ``rows`` rows.  Row r continues slot r from the
    same prompt with ITS OWN next token, so a step of B rows is B samples:
    for a single next token the K error is a coin flip between the formats
    (V's e4m3 rounding, the same in both, is as large), and B copies of one
    row would measure that one token B times.  ``against``: "fp32" (the
    reference model) or "bf16" (the same engine with a bf16 cache)."""
    if against == "bf16":
        a = _step_logits(ckpt, kv, device, rows, prompt)
        b = _step_logits(ckpt, "bf16", device, rows, prompt)
        return {k: float((a[k] - b[k]).abs().max()) / float(b[k].abs().max()) for k in a}
    nslots = max(rows)
    m = LocalLM.load_safetensors(ckpt, device=device, max_batch=nslots, max_rows=nslots, max_seq=64, kv_dtype=kv)
    toks = _tokens(prompt, 1)
    nxt = _tokens(nslots, 2)
    refs = {t: m.reference_logits(toks + [t]).float().cpu() for t in sorted(set(nxt))}
    out = {}
    got = m.forward_tokens(torch.tensor(toks, dtype=torch.int32), 0, 0).float().cpu()
    ref0 = refs[nxt[0]][prompt - 1]
    out["prefill"] = float((got - ref0).abs().max()) / float(ref0.abs().max())
    m.fork_kv(0, list(range(1, nslots)), 0, prompt)
    for B in rows:
        t = torch.tensor(nxt[:B], dtype=torch.int32, device=device)
        sl = torch.arange(B, dtype=torch.int32, device=device)
        pos = torch.full((B,), prompt, dtype=torch.int32, device=device)
        lg = m.decode(t, sl, pos).float().cpu()
        ref = torch.stack([refs[x][prompt] for x in nxt[:B]])
        out[f"decode {B} rows"] = float((lg - ref).abs().max()) / float(ref.abs().max())
    return out


def _step_logits(ckpt: str, kv: str, device: str, rows, prompt: int) -> dict:
    """The logits :func:`step_errors` measures, themselves."""
    nslots = max(rows)
    m = LocalLM.load_safetensors(ckpt, device=device, max_batch=nslots, max_rows=nslots, max_seq=64, kv_dtype=kv)
    toks, nxt = _tokens(prompt, 1), _tokens(nslots, 2)
    out = {"prefill": m.forward_tokens(torch.tensor(toks, dtype=torch.int32), 0, 0).float().cpu()}
    m.fork_kv(0, list(range(1, nslots)), 0, prompt)
    for B in rows:
        t = torch.tensor(nxt[:B], dtype=torch.int32, device=device)
        sl = torch.arange(B, dtype=torch.int32, device=device)
        pos = torch.full((B,), prompt, dtype=torch.int32, device=device)
        out[f"decode {B} rows"] = m.decode(t, sl, pos).float().cpu()
    return out

"""A tiny written Mistral checkpoint (window 24, slots of 256 positions) on the
GPU: batched prefill behind a shared prefix, then 40 decode steps replayed
from one captured graph -- three rows per step, one of them a forked branch
that reads its parent's keys in place -- against ``reference_logits`` in fp32
on the CPU, for each KV format.  The per-row cosine bound and the decisive
top-1 rule are those of tests/test_gpu_qkv_bias.py (0.999 bf16, 0.99 fp8; the
per-row scaled format is held to fp8's).  The captured decode graph of the
windowed model has as many kernel nodes as its full-attention twin's."""
import pytest
import torch

from tests.test_gpu_qkv_bias import _check_rows

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

WINDOW, MAX_SEQ, P, STEPS = 24, 256, 30, 40


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    from dmcp.utils import synth
    return synth.llama_checkpoint(str(tmp_path_factory.mktemp("mistral_tiny")), layers=2, hidden=256, heads=4,
                                  kv_heads=2, intermediate=512, vocab=512, tokenizer="", outliers=(7,),
                                  model_type="mistral", sliding_window=WINDOW, device="cpu")


@pytest.fixture(scope="module")
def ref(ckpt):
    """Tokens and fp32 CPU logits of the three logical sequences (computed once)."""
    from dmcp.models.llm import LocalLM
    cpu = LocalLM.load_safetensors(ckpt, device="cpu", max_seq=MAX_SEQ, max_batch=1, max_rows=1)
    assert cpu.windows == (WINDOW, WINDOW)
    g = torch.Generator().manual_seed(9)
    prefix = torch.randint(0, 512, (P,), generator=g).tolist()
    pa, pb = (torch.randint(0, 512, (n,), generator=g).tolist() for n in (17, 41))
    streams = [torch.randint(0, 512, (STEPS,), generator=g).tolist() for _ in range(3)]
    # slot 0: prefix + pa + stream 0; slot 1: a branch of slot 0 forked after pa; slot 2: prefix + pb + stream 2
    seqs = [prefix + pa + streams[0], prefix + pa + streams[1], prefix + pb + streams[2]]
    return prefix, pa, pb, streams, [cpu.reference_logits(s) for s in seqs]


def _run(ckpt, ref, kv, windows=True):
    """(prefill logits, decode logits [STEPS, 3, V], kernel nodes of the decode graph)."""
    from dmcp.models.llm import LocalLM, graph_kernel_nodes
    prefix, pa, pb, streams, _ = ref
    over = {} if windows else dict(layer_windows=None)
    m = LocalLM.load_safetensors(ckpt, device="cuda", max_seq=MAX_SEQ, max_batch=4, max_rows=8, kv_dtype=kv, **over)
    assert (m.windows == (WINDOW, WINDOW)) if windows else (m.windows is None)
    assert m.set_prefix(prefix) == P
    for s in (0, 2):
        m.fork_prefix(s)
    pre = m.prefill_batch([(pa, 0, P), (pb, 2, P)])
    m.fork_share(0, [1], P + len(pa))
    start = [P + len(pa), P + len(pa), P + len(pb)]
    tk = torch.zeros(3, dtype=torch.int32, device="cuda")
    ps = torch.zeros(3, dtype=torch.int32, device="cuda")
    sl = torch.arange(3, dtype=torch.int32, device="cuda")

    def feed(j):
        tk.copy_(torch.tensor([streams[r][j] for r in range(3)], dtype=torch.int32))
        ps.copy_(torch.tensor([start[r] + j for r in range(3)], dtype=torch.int32))
    feed(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture (step 0 is replayed below: same cache rows)
        m.decode(tk, sl, ps)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        out = m.decode(tk, sl, ps)
    g.instantiate()
    nodes = graph_kernel_nodes(g)
    got = []
    for j in range(STEPS):
        feed(j)
        g.replay()
        got.append(out.float().clone())
    torch.cuda.synchronize()
    return pre, torch.stack(got), nodes


@pytest.mark.parametrize("kv,bound", [("bf16", 0.999), ("fp8", 0.99), ("fp8s", 0.99)])
def test_windowed_checkpoint_prefills_and_decodes(ckpt, ref, kv, bound):
    prefix, pa, pb, streams, logits = ref
    pre, dec, nodes = _run(ckpt, ref, kv)
    exp = torch.stack([logits[0][P + len(pa) - 1], logits[2][P + len(pb) - 1]])
    _check_rows(pre, exp, bound, f"windowed prefill {kv}")
    start = [P + len(pa), P + len(pa), P + len(pb)]
    exp = torch.stack([torch.stack([logits[r][start[r] + j] for r in range(3)]) for j in range(STEPS)])
    _check_rows(dec.reshape(-1, dec.shape[-1]), exp.reshape(-1, exp.shape[-1]), bound, f"windowed decode {kv}")
    # the window matters on these inputs: the full-attention twin misses the same bound
    _, full, full_nodes = _run(ckpt, ref, kv, windows=False)
    cos = torch.nn.functional.cosine_similarity(full.reshape(-1, full.shape[-1]).cpu(),
                                                exp.reshape(-1, exp.shape[-1]), dim=-1)
    print(f"full-attention twin {kv}: min cosine {cos.min().item():.5f}; kernel nodes {nodes} / {full_nodes}")
    assert cos.min().item() < bound
    assert nodes == full_nodes and nodes > 0

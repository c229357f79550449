"""The worker witness (dmcp/enrich/workers.py) reports the KV-cache format, so
a checkpoint left on the saturating fp8 default shows in the start log."""
import pytest

from dmcp.enrich import workers
from dmcp.models.llm import LocalLM, preset


@pytest.mark.parametrize("kv", ["bf16", "fp8", "fp8s"])
def test_witness_reports_the_cache_format(kv):
    m = LocalLM(preset("tiny", max_batch=2, max_seq=64, kv_dtype=kv), device="cpu")
    w = workers._witness("cpu", m)
    assert w == {"device": "cpu", "kv_dtype": kv}


def test_witness_without_a_model_is_unchanged():
    assert workers._witness("cpu") == {"device": "cpu"}

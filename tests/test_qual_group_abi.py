"""The exact and the flat qualified calls under a group rule are, in include/vsgpu.h, the ungrouped ones with per_group after k."""
import pytest

from test_grouped_abi import params


@pytest.mark.parametrize("plain", ["vs_search_batch_qual_exact", "vs_search_batch_qual_exact_dev", "vs_search_batch_qual_flat",
                                   "vs_search_batch_qual_flat_dev"])
def test_the_grouped_prototype_adds_per_group_after_k(plain):
    want = params(plain)
    want.insert(want.index("uint32_t k") + 1, "uint32_t per_group")
    grouped = plain.replace("_dev", "") + "_grouped" + ("_dev" if plain.endswith("_dev") else "")
    assert params(grouped) == want

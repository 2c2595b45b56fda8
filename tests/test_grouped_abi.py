"""The grouped batch calls of include/vsgpu.h are the qualified ones with per_group after k; the sentinel and the option are named."""
import os
import re

import pytest

HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vsgpu.h")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)


def params(name):
    args = re.search(r"\bint %s\s*\((.*?)\);" % name, CODE, flags=re.S).group(1)
    return [re.sub(r"\s+", " ", a).strip().replace("d_qual_slots", "qual_slots") for a in args.split(",")]


@pytest.mark.parametrize("qual,grouped", [("vs_search_batch_qual", "vs_search_batch_grouped"), ("vs_search_batch_dev_qual", "vs_search_batch_dev_grouped"),
                                          ("vs_search_batch_dev_qual_finish", "vs_search_batch_dev_grouped_finish")])
def test_the_grouped_prototype_adds_per_group_after_k(qual, grouped):
    want = params(qual)
    if "uint32_t k" in want:
        want.insert(want.index("uint32_t k") + 1, "uint32_t per_group")
    assert params(grouped) == want


def test_the_sentinel_and_the_option_are_in_the_header():
    assert re.search(r"#define VS_GROUP_NONE 0xFFFFFFFFu\b", CODE) and "VS_GROUP_FIRST_POPS" in HEADER
    from pgvectorscale_amd import _lib
    assert _lib.GROUP_NONE == 0xFFFFFFFF

"""The public face of the latency-mode search kernel: one enum value appended to the line that names the search kernels, mirrored in
_lib.py, and its options documented where every option is — no new function, struct or field."""
import os
import re

import pytest

from pgvectorscale_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTIONS = ["VS_LAT_SCANS", "VS_LAT_WAVES", "VS_LAT_SPEC", "VS_LAT_CACHE", "VS_LAT_HEAP_LDS", "VS_LAT_HEAP_CAP", "VS_LAT_DEDUP_SLOTS",
           "VS_LAT_VISITED"]


def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_enum_value():
    assert "enum { VS_SEARCH_GENERAL = 0, VS_SEARCH_FAST_SBQ = 1, VS_SEARCH_FAST_PLAIN = 2, VS_SEARCH_LAT_SBQ = 3 };" in _read("include", "vsgpu.h")
    assert _lib.VS_SEARCH_LAT_SBQ == 3


@pytest.mark.parametrize("option", OPTIONS)
def test_option_is_documented(option):
    header = _read("include", "vsgpu.h")
    comment = header[header.index("/* Tuning options"):header.index("int vs_set_option")]
    assert re.search(r"\b%s\b" % option, comment), "not in the option comment of include/vsgpu.h"
    design = _read("DESIGN.md")
    sec10 = design[design.index("\n## 10"):]
    assert re.search(r"`%s`" % option, sec10), "not in DESIGN.md section 10"

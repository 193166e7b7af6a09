"""tsdbhip_debug_buffers, the read-out of the library's live device and page-locked host buffers
(csrc/devbuf.h): it takes no context, so it answers without a GPU.  What the counters count is
checked on the device (tests/test_gpu_buffers.py)."""
from __future__ import annotations

import os
import re

from opentsdb_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opentsdb_amd", "csrc")


def test_four_non_negative_integers():
    got = E.debug_buffers()
    assert len(got) == 4
    assert all(isinstance(v, int) and v >= 0 for v in got), got


def test_two_calls_agree():
    assert E.debug_buffers() == E.debug_buffers()


def test_null_pointers():
    assert E.lib().tsdbhip_debug_buffers(None, None, None, None) == 0


def test_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "tsdbhip.h")).read()
    assert "int tsdbhip_debug_buffers(int64_t* dev_n, uint64_t* dev_bytes, int64_t* host_n, uint64_t* host_bytes);" in hdr
    assert "tsdbhip_debug_buffers" in E.EXPORTS


def test_one_buffer_type_and_no_hand_written_scope_guards():
    # the buffers are devbuf.h's in every translation unit that holds any (multi.cpp's Buf is another
    # thing: it switches device), and nothing frees them by a guard of its own
    hits = []
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".cpp", ".h", ".hip")) and f != "devbuf.h":
            for i, ln in enumerate(open(os.path.join(CSRC, f)), 1):
                if re.search(r"struct (DevBuf|HostBuf|Drop|Rel|Hold)\b|frees nothing on its own", ln):
                    hits.append(f"{f}:{i}")
    assert not hits, hits

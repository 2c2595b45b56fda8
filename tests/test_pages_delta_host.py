"""The page-by-page write-back (vs_pages_out_baseline / _delta / _read_blocks) and vs_index_bulk_delete without a GPU: the cases of
tests/test_gpu_zzzz_pages_delta.py and tests/test_gpu_zv_bulk_delete.py run in a child process on the wave64 lockstep interpreter
(VS_EMU=1, as tests/test_pages_write_host.py runs the writer's) — the unmodified kernel sources, the digest's in-wave shuffles and
its cross-wave sum through LDS included.  One ABI case of its own: a baseline outlives its writer and its index."""
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_LIB = os.path.join(EMU_DIR, "libvsgpu_emu.so")


def _build_emu():
    r = subprocess.run(["make", "-C", EMU_DIR, "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("module", ["test_gpu_zzzz_pages_delta.py", "test_gpu_zv_bulk_delete.py"])
def test_gpu_cases_pass_on_the_wave64_interpreter(module):
    if os.environ.get("VS_EMU"):
        pytest.skip("already inside the emulated run")
    _build_emu()
    env = dict(os.environ, VS_EMU="1")
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", module), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT, timeout=3000)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail


def test_a_baseline_outlives_its_writer_and_its_index():
    """vs_pages_base belongs to the device, not to the vs_pages_out or the vs_index it was taken from: still readable, still good
    for a delta on another index, and freed safely after both are gone"""
    if os.environ.get("VS_EMU"):
        pytest.skip("already inside the emulated run")
    _build_emu()
    script = textwrap.dedent("""
        import numpy as np
        import pgvectorscale_amd as P
        from pgvectorscale_amd.pages import PagesOut
        n, W, R = 200, 2, 8
        rng = np.random.default_rng(1)
        nbrs = np.full((n, R), 0xFFFFFFFF, np.uint32)
        for i in range(n):
            nbrs[i, :3] = [(i + 1) % n, (i + 7) % n, (i + 31) % n]
        kw = dict(codes=rng.integers(0, 1 << 62, (n, W), dtype=np.uint64), nbrs=nbrs,
                  heap_tids=(np.arange(1, n + 1, dtype=np.uint64) << np.uint64(16)) | np.uint64(1), vecs=rng.random((n, 64), dtype=np.float32),
                  mean=np.zeros(64, np.float32), m2=np.ones(64, np.float32), count=n, bits=2, dim_index=64, num_neighbors=R,
                  distance_type=P.VS_L2, default_start=0)
        ctx = P.Context(0)
        ix = P.DiskAnnIndex.upload(ctx, **kw)
        out = PagesOut(ix)
        nb = out.n_blocks
        base = out.baseline()
        out.close()
        ix.close()
        assert base.n_blocks == nb > 2
        ix2 = P.DiskAnnIndex.upload(ctx, **kw)          # the same arrays somewhere else in memory
        ix2.mark_deleted(np.array([n - 1], np.uint32))
        out2 = PagesOut(ix2)
        blocks, nb_now, base2 = out2.delta(base)
        assert blocks.tolist() == [out2.item_pointer_of(n - 1)[0]] and nb_now == nb
        out2.close()
        ix2.close()
        base.close()
        base2.close()
        base2.close()                                     # (closing twice is a no-op)
        ctx._L.vs_pages_base_free(None)
        assert ctx._L.vs_pages_base_blocks(None) == 0
        ctx.close()
        print("baseline ok")
    """)
    env = dict(os.environ, VS_LIB_PATH=EMU_LIB, VS_NO_TORCH="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and "baseline ok" in r.stdout, (r.stdout + r.stderr)[-3000:]

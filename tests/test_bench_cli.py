"""bench.py's own options: a plain run times exactly --steps steps and prints the headline only (the rest is --full's),
and --dump-outputs writes what the last timed step handed its caller, within 64 MB."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _fake_step(torch, nblk, bs, slot):
    """Host tensors shaped like a step's outputs: block b's stream is slot bytes long at most, its decoded bytes bs."""
    rs = np.random.RandomState(3)
    csz = rs.randint(1, slot + 1, size=nblk).astype(np.int32)
    comp = torch.from_numpy(rs.randint(0, 256, size=nblk * slot).astype(np.uint8))
    back = torch.from_numpy(rs.randint(0, 256, size=nblk * bs).astype(np.uint8))
    z = torch.zeros(nblk, dtype=torch.int32)
    return comp, torch.from_numpy(csz), z, back, torch.full((nblk,), bs, dtype=torch.int32), z.clone()


def test_dump_outputs_writes_the_callers_arrays(tmp_path):
    import torch
    import bench
    nblk, bs, slot = 50, 4096, 1280
    comp, csz, st_e, back, bsz, st_d = _fake_step(torch, nblk, bs, slot)
    bench.dump_outputs(str(tmp_path), nblk, bs, slot, comp, csz, st_e, back, bsz, st_d)
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(got) == {"block_index", "comp_size", "enc_status", "dec_size", "dec_status", "sample_blocks",
                        "comp_bytes", "dec_bytes"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["comp_size"], csz.numpy()) and np.array_equal(got["dec_size"], bsz.numpy())
    sample = got["sample_blocks"].astype(int)
    assert sample[0] == 0 and sample[-1] == nblk - 1
    want_c = np.concatenate([comp.numpy()[b * slot:b * slot + int(csz[b])] for b in sample])
    want_d = np.concatenate([back.numpy()[b * bs:(b + 1) * bs] for b in sample])
    assert np.array_equal(got["comp_bytes"], want_c) and np.array_equal(got["dec_bytes"], want_d)
    # the same arguments give the same files
    again = tmp_path / "again"
    bench.dump_outputs(str(again), nblk, bs, slot, comp, csz, st_e, back, bsz, st_d)
    assert all(np.array_equal(np.load(again / (k + ".npy")), v) for k, v in got.items())


def test_dump_outputs_samples_within_the_limit(tmp_path, monkeypatch):
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT", 40000)
    nblk, bs, slot = 20, 8192, 2048
    comp, csz, st_e, back, bsz, st_d = _fake_step(torch, nblk, bs, slot)
    bench.dump_outputs(str(tmp_path), nblk, bs, slot, comp, csz, st_e, back, bsz, st_d)
    total = sum(np.load(tmp_path / f).nbytes for f in os.listdir(tmp_path))
    assert 0 < total <= 40000
    dec = np.load(tmp_path / "dec_bytes.npy")
    assert 0 < dec.size < 8 * bs


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps(tmp_path, oracle):
    """A plain run: the headline keys, exactly --steps timed steps, nothing of --full; the dump holds the last step's
    streams (bit-equal to the oracle's) and decoded bytes (equal to the input)."""
    import bench
    out_dir = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--blocks", "600", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
    assert not {"roofline", "gate", "configs4", "hetero", "host_path", "cpu_baseline"} & set(out)
    got = {f[:-4]: np.load(out_dir / f) for f in os.listdir(out_dir)}
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert (got["enc_status"] == 0).all() and (got["dec_status"] == 0).all() and got["comp_size"].size == 600
    bs = out["config"]["block_size"]
    pos = 0
    for i, b in enumerate(got["sample_blocks"].astype(int)):
        n = int(got["comp_size"][b])
        raw = bench.block_bytes("q40+dir", bs, b).tobytes()
        assert got["comp_bytes"][pos:pos + n].astype(np.uint8).tobytes() == oracle.compress(raw, 1), b
        assert got["dec_bytes"][i * bs:(i + 1) * bs].astype(np.uint8).tobytes() == raw, b
        pos += n
    assert pos == got["comp_bytes"].size

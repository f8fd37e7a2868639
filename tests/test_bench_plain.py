"""A plain `bench.py` run (no --full) times the headline workload and nothing else, and --dump-outputs writes what its last timed
step computed: checked here against the synthetic inputs (decode returns them) and the oracle's tile bytes (encode)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


@pytest.mark.gpu
def test_plain_line_is_lean_and_dump_outputs_is_the_last_step(tmp_path):
    from oracle import pyoracle as po
    from xpng_amd.synth import synth_raster
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    share, batch, steps = 1024, 3, 5
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--share", str(share), "--batch", str(batch), "--pipeline", "2",
                          "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(tmp_path / "dump")],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["metric"] == "Mpixels/s encode+decode (bit-exact vs ref)" and line["unit"] == "Mpx/s"
    assert line["higher_is_better"] is True and line["dtype"] == "u8" and line["steps"] == steps
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] - batch * share * share / (line["ms_per_step"] * 1e3)) <= 0.01 * line["value"]
    for moved in ("verified", "roofline", "step_roofline", "cpu_baseline", "single_image", "legs", "config4"):
        assert moved not in line, moved

    d = {n[:-4]: np.load(tmp_path / "dump" / n) for n in os.listdir(tmp_path / "dump")}
    assert set(d) == {"blob_lengths", "blob_byte_sums", "blob_sample", "decoded_channel_sums", "decoded_sample"}
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert sum(a.nbytes for a in d.values()) <= 64 << 20
    rng = np.random.default_rng(20240611)   # bench.py DUMP_SEED: the sample positions, as fractions of each output
    u_blob, u_rast = rng.random((1 << 20) // batch), rng.random((1 << 22) // batch)
    for b in range(batch):
        raster = synth_raster("photo", share, share, True, seed=1 + b)
        blobs = np.frombuffer(po.encode_tiles(1, raster), dtype=np.uint8)
        assert d["blob_lengths"][b] == len(blobs) and d["blob_byte_sums"][b] == blobs.sum(dtype=np.int64)
        assert np.array_equal(d["blob_sample"][b], blobs[(u_blob * len(blobs)).astype(np.int64)].astype(np.float32))
        flat = raster.reshape(-1)
        assert np.array_equal(d["decoded_channel_sums"][b], raster.reshape(-1, 4).sum(0, dtype=np.int64).astype(np.float64))
        assert np.array_equal(d["decoded_sample"][b], flat[(u_rast * flat.size).astype(np.int64)].astype(np.float32))

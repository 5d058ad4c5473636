"""bench.py launcher on the CPU (gloo): ``--gpus N`` starts N ranks by itself, every
rank sees WORLD_SIZE == N, the JSON reports the world actually seen, the frame
count is the sum over ranks of the timed steps, and a failing rank ends the job
with a non-zero status naming the rank."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(**kw):
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="2")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    env.update(kw)
    return env


ARGS = ["--steps", "2", "--warmup", "1", "--tiny", "--batch", "3", "--pool", "3"]


def _expected_frames(world, steps=2, warm=1, batch=3, pool=3):
    from speakingstyle_amd.data.synthetic import SyntheticBatches

    total = 0
    for r in range(world):
        gen = SyntheticBatches(batch, seed=1000 + r, max_seq_len=1000)
        ps = []
        for _ in range(pool):
            b = gen.make_batch()
            ps.append((len(b[0]) * b[8], gen.last_valid_frames))
        ps.sort(key=lambda e: -e[0])
        total += sum(ps[(warm + i) % pool][1] for i in range(steps))
    return total


def test_bench_launches_two_ranks():
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--full", "--synth-batch", "2", "--synth-steps", "2",
                        "--synth-b1-runs", "3"] + ARGS,
                       cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 only
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["world_size_seen"] == 2
    assert rec["config"]["parallelism"] == "dp2" and rec["config"]["global_batch"] == 6
    assert rec["bucket_overlap"] is True
    frames = rec["value"] * rec["ms_per_step"] * rec["steps"] / 1000.0
    np.testing.assert_allclose(frames, _expected_frames(2), rtol=2e-3)
    assert rec["synth_rtf"] > 0 and rec["synth"]["batch_per_gpu"] == 2 and rec["synth"]["distinct_batches"] == 2
    b1 = rec["synth"]["b1"]  # batch-1 latency (like-for-like with the reference's 113-frame point)
    assert rec["synth_rtf_b1"] > 0 and b1["runs"] == 3 and b1["mel_frames"] > 0
    assert rec["synth_vs_baseline"] == round(1.33 / rec["synth_rtf_b1"], 1)


def test_bench_single_process_default():
    r = subprocess.run([sys.executable, "bench.py", "--synth-steps", "0"] + ARGS, cwd=ROOT, env=_env(),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["n_gpus"] == 1 and "synth_rtf" not in rec
    frames = rec["value"] * rec["ms_per_step"] * rec["steps"] / 1000.0
    np.testing.assert_allclose(frames, _expected_frames(1, warm=1), rtol=2e-3)


def test_bench_plain_run_and_output_dump(tmp_path):
    """Without ``--full`` the synthesis options are inert (training headline only); ``--dump-outputs`` writes the
    last timed step's results as float32 / float64 .npy files, the same from run to run."""
    dumps = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, "bench.py", "--synth-batch", "2", "--synth-steps", "2",
                            "--dump-outputs", str(tmp_path / d)] + ARGS, cwd=ROOT, env=_env(),
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        assert "synth_rtf" not in rec and "synth" not in rec
        assert rec["steps"] == 2 and rec["ms_per_step"] > 0 and rec["unit"] == "mel-frames/s"
        files = sorted(os.listdir(tmp_path / d))
        dumps.append({f: np.load(tmp_path / d / f) for f in files})
    a, b = dumps
    assert sorted(a) == sorted(b) and "lr.npy" in a
    assert sum(1 for f in a if f.startswith("loss_")) == 6 and "output_0.npy" in a and "output_1.npy" in a
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for f in a:
        assert a[f].dtype in (np.float32, np.float64), f
        assert np.isfinite(a[f]).all(), f
        np.testing.assert_allclose(a[f], b[f], rtol=1e-5, atol=1e-6, err_msg=f)
    assert a["output_1.npy"].ndim == 3 and a["output_1.npy"].shape[0] == 3  # [batch, frames, mel bins]


def test_dump_outputs_samples_large_arrays(tmp_path, monkeypatch):
    import torch

    from speakingstyle_amd import benchmark as B

    monkeypatch.setattr(B, "DUMP_BUDGET_BYTES", 4096)
    big = torch.arange(10000, dtype=torch.float32).reshape(100, 100)
    mask = torch.arange(10000).reshape(100, 100) % 2 == 0
    result = ([torch.tensor(1.5)], (big, None, mask, 7), 1e-3)
    B.dump_outputs(str(tmp_path / "a"), result)
    B.dump_outputs(str(tmp_path / "b"), result)
    got = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["loss_0.npy", "lr.npy", "output_0.npy", "output_2.npy"]
    assert got["loss_0.npy"] == np.float32(1.5) and got["lr.npy"] == 1e-3
    o0, o2 = got["output_0.npy"], got["output_2.npy"]
    # the scalar is stored whole (4 bytes); the two large arrays share what is left evenly
    assert o0.dtype == np.float32 and o0.shape == (4092 // 2 // 4,) and (np.diff(o0) > 0).all()  # sorted flat indices
    assert o2.dtype == np.float64 and o2.shape == (2048 // 8,) and set(np.unique(o2)) <= {0.0, 1.0}
    assert sum(v.nbytes for v in got.values()) <= 4096 + 8  # + lr
    for f in got:
        np.testing.assert_array_equal(got[f], np.load(tmp_path / "b" / f))


def test_bench_failing_rank_exits_nonzero():
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--synth-steps", "0"] + ARGS, cwd=ROOT,
                       env=_env(SSAMD_EXPERIMENTAL="fail_rank=1", SSAMD_DIST_TIMEOUT_S="60"), capture_output=True, text=True,
                       timeout=900)
    assert r.returncode != 0
    assert "[rank 1] FAILED" in r.stderr and "injected failure on rank 1" in r.stderr


def test_world_size_mismatch_is_an_error():
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "3", "--synth-steps", "0"] + ARGS, cwd=ROOT,
                       env=_env(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"), capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "3 ranks were requested" in r.stderr


def test_slurm_job_script_syntax():
    """scripts/train_job.sh (the reference's scripts/train_job.sh counterpart): valid bash,
    one torchrun rank per GPU, RCCL env set; a full 2-rank CPU run of it is in docs (slow)."""
    import subprocess

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "train_job.sh")
    subprocess.run(["bash", "-n", path], check=True)
    text = open(path).read()
    assert "torch.distributed.run" in text and "--nproc-per-node" in text
    assert "HSA_ENABLE_IPC_MODE_LEGACY=0" in text and "#SBATCH --gres=gpu:8" in text

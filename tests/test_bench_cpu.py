"""Host-side pieces of bench.py (no GPU): the stall watchdog and the a-priori link arithmetic of the N > 1 line, the options
and the output dump."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_link_bound_estimate_arithmetic():
    import bench
    assert bench.link_bound_estimate(2_620_000_000, 1, 5.9) is None
    e = bench.link_bound_estimate(2_620_000_000, 8, 5.9)
    # 2 (N - 1) / N of the gradient bytes cross every rank's links: 4.585 GB at N = 8
    assert e['bytes_per_rank_on_the_wire'] == int(2.0 * 7 / 8 * 2_620_000_000)
    assert e['all_links_ms'] == pytest.approx(1e3 * e['bytes_per_rank_on_the_wire'] / (7 * 153e9))
    assert e['single_ring_ms'] == pytest.approx(3.5 * e['all_links_ms'])
    assert 0.0 < e['weak_scaling_ceiling_if_fully_exposed'] < 1.0
    e2 = bench.link_bound_estimate(2_620_000_000, 2, 5.9)
    assert e2['all_links_ms'] == pytest.approx(1e3 * 2_620_000_000 / 153e9)      # one peer: one link


def test_watchdog_ends_a_stalled_rank_with_code_3():
    """A rank that stops beating exits by itself (code 3) -- the launcher (and torch.distributed.run) then tear the job down;
    a rank that keeps beating is left alone."""
    code = ("import sys, time; sys.path.insert(0, %r); import bench\n"
            "d = bench.Watchdog(1.5, 0)\n"
            "for _ in range(8):\n"
            "    time.sleep(0.3); d.beat('loop')\n"
            "print('alive', flush=True)\n"
            "time.sleep(30)\n" % ROOT)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3, (r.returncode, r.stderr[-500:])
    assert 'alive' in r.stdout and 'no progress' in r.stderr and 'loop' in r.stderr


def test_dump_sample_positions_are_fixed_and_in_range():
    """--dump-outputs samples large flat buffers at seeded positions: the same in every run, sorted, inside the buffer."""
    import numpy as np
    import bench
    a = bench.sample_positions(10 ** 8, 1)
    assert np.array_equal(a, bench.sample_positions(10 ** 8, 1))
    assert len(a) == bench.DUMP_SAMPLE and a.min() >= 0 and a.max() < 10 ** 8 and (np.diff(a) >= 0).all()
    assert not np.array_equal(a, bench.sample_positions(10 ** 8, 2))
    assert np.array_equal(bench.sample_positions(1000, 1), np.arange(1000))       # small buffers: every element


def test_write_outputs_writes_float_arrays_within_the_limit(tmp_path):
    import numpy as np
    import bench
    bench.write_outputs(str(tmp_path / 'o'), {'a': np.arange(5, dtype=np.float32), 'b': np.ones(3)})
    assert np.array_equal(np.load(tmp_path / 'o' / 'a.npy'), np.arange(5, dtype=np.float32))
    assert np.load(tmp_path / 'o' / 'b.npy').dtype == np.float64
    with pytest.raises(SystemExit):
        bench.write_outputs(str(tmp_path / 'p'), {'big': np.zeros(bench.DUMP_LIMIT // 8 + 1)})
    assert not (tmp_path / 'p').exists()


def test_bench_options():
    """--full and --dump-outputs exist; --steps sets the number of timed steps and must be at least one."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--help'], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and '--full' in r.stdout and '--dump-outputs' in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and '--steps' in r.stderr

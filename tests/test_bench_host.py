"""Host logic of bench.py that runs without a GPU: the live roofline.traffic measurement's counter parsing and the
algorithmic bytes per block."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_counter_bytes_per_launch_sums_dimensions_and_averages_dispatches():
    b = _bench()
    k = b.HEADLINE_KERNEL
    rows = [
        # dispatch 1: two instance rows (summed), dispatch 2: one row; another kernel and another counter are ignored
        {"Dispatch_Id": "1", "Kernel_Name": f"void (anonymous namespace)::{k}(pba::detail::KernelArgs)",
         "Counter_Name": "FETCH_SIZE", "Counter_Value": "100.0"},
        {"Dispatch_Id": "1", "Kernel_Name": f"void (anonymous namespace)::{k}(pba::detail::KernelArgs)",
         "Counter_Name": "FETCH_SIZE", "Counter_Value": "50.0"},
        {"Dispatch_Id": "2", "Kernel_Name": f"void (anonymous namespace)::{k}(pba::detail::KernelArgs)",
         "Counter_Name": "FETCH_SIZE", "Counter_Value": "250.0"},
        {"Dispatch_Id": "3", "Kernel_Name": "void linearize_kernel<0, 0, 8>(...)", "Counter_Name": "FETCH_SIZE",
         "Counter_Value": "9999.0"},
        {"Dispatch_Id": "2", "Kernel_Name": f"{k}", "Counter_Name": "WRITE_SIZE", "Counter_Value": "7.0"},
    ]
    assert b.counter_bytes_per_launch(rows, "FETCH_SIZE", k) == (150.0 + 250.0) / 2 * 1024.0
    assert b.counter_bytes_per_launch(rows, "WRITE_SIZE", k) == 7.0 * 1024.0
    assert b.counter_bytes_per_launch(rows, "GRBM_COUNT", k) is None


def test_dump_outputs_writes_a_fixed_sample_within_64_mb(tmp_path):
    """--dump-outputs at the headline's size (400k blocks x 112 floats): float32 / float64 .npy files, at most 64 MB in
    all, the same seeded sample of blocks on every call."""
    import numpy as np
    b = _bench()

    class FakeEngine:
        n, rec = 400000, 112

        def records(self):
            r = np.arange(self.n, dtype=np.float32)[:, None] + np.zeros((1, self.rec), np.float32)
            return r, (np.arange(self.n) % 7 != 0).astype(np.uint8)

        def block_costs(self):
            return np.arange(self.n, dtype=np.float32) * 0.5

    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    for d in dirs:
        b.dump_outputs(FakeEngine(), d)
    names = sorted(os.listdir(dirs[0]))
    assert names == ["block_costs.npy", "record_blocks.npy", "records.npy", "valid.npy"]
    arrays = {n: np.load(os.path.join(dirs[0], n)) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 1000 * 1000
    for n in names:
        assert np.array_equal(arrays[n], np.load(os.path.join(dirs[1], n)))
    sel = arrays["record_blocks.npy"].astype(np.int64)
    assert sel.shape == (b.DUMP_BLOCKS,) and np.all(np.diff(sel) > 0) and sel[-1] < 400000
    assert np.array_equal(arrays["records.npy"][:, 0], sel.astype(np.float32))  # the sampled blocks' own records
    assert arrays["valid.npy"].shape == (400000,) and set(np.unique(arrays["valid.npy"])) == {0.0, 1.0}
    assert np.array_equal(arrays["block_costs.npy"], np.arange(400000, dtype=np.float32) * 0.5)


def test_algorithmic_bytes_per_block_at_c4():
    b = _bench()
    # 517.3 B at P = 8, K = 4 on the C4 problem
    v = b.algorithmic_bytes_per_block(8, 4, 1004, 100000, 400000)
    assert abs(v - 517.28) < 0.01

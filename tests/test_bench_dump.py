"""bench.py --dump-outputs: the arrays written for a front end's last step (CPU only;
a stand-in front end with the three read-back calls the dump uses)."""
import os

import numpy as np

import bench


class FakeFrontend:
    def __init__(self, counts):
        self.counts = counts

    def pose(self, s):
        return np.full(3, s + 0.25), np.full(3, -s - 0.5)

    def features(self, s):
        n = self.counts[s]
        return (np.arange(2 * n, dtype=np.float32).reshape(n, 2) + s)

    def map_points(self, s):
        n = self.counts[s]
        return np.arange(3 * n, dtype=np.float64).reshape(n, 3) - s


STATS = {"lk_iterations": 7, "tracked": 6, "inliers": 5, "added": 4, "features": 3, "keyframes": 2, "hypotheses": 99}


def load(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_dump_outputs_layout(tmp_path):
    counts = [3, 0, 5]
    bench.dump_outputs(str(tmp_path / "d"), FakeFrontend(counts), 3, 4, STATS)
    d = load(str(tmp_path / "d"))
    assert sorted(d) == ["counts", "features", "map_points", "poses", "step_counts"]
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert d["poses"].shape == (3, 6) and d["poses"][2].tolist() == [2.25] * 3 + [-2.5] * 3
    assert d["counts"].tolist() == counts
    # the capacity is n_features, or the largest count above it; rows past a count are zero
    assert d["features"].shape == (3, 5, 2) and d["map_points"].shape == (3, 5, 3)
    fe = FakeFrontend(counts)
    for s, n in enumerate(counts):
        assert np.array_equal(d["features"][s, :n], fe.features(s)) and not d["features"][s, n:].any()
        assert np.array_equal(d["map_points"][s, :n], fe.map_points(s)) and not d["map_points"][s, n:].any()
    assert d["step_counts"].tolist() == [7, 6, 5, 4, 3, 2]


def test_dump_outputs_stays_under_64_mb(tmp_path):
    """A batch over 64 MB is cut to its first sequences (4k: 16000 features, 256 sequences)."""
    n_seq, n_feat = 256, 16000
    bench.dump_outputs(str(tmp_path / "d"), FakeFrontend([1] * n_seq), n_seq, n_feat, STATS)
    d = load(str(tmp_path / "d"))
    keep = len(d["poses"])
    assert 0 < keep < n_seq and all(len(d[k]) == keep for k in ("counts", "features", "map_points"))
    assert sum(a.nbytes for a in d.values()) <= bench.DUMP_MAX_BYTES
    assert sum(os.path.getsize(os.path.join(str(tmp_path / "d"), f)) for f in os.listdir(str(tmp_path / "d"))) <= bench.DUMP_MAX_BYTES
    # one more sequence would not have fitted
    per_seq = sum(d[k][0].nbytes for k in ("poses", "counts", "features", "map_points"))
    assert (keep + 1) * per_seq > bench.DUMP_MAX_BYTES - 4096


def test_ring_index_follows_the_scene_cycle():
    """Past RING_FRAMES the steps wrap to ring frames of the same phase of the scenes'
    cycle, each step's previous ring frame holding what the previous step's frame held."""
    # the wrap keeps the frame's phase and the library's t mod 2 / t mod 3 buffer keys
    assert bench.RING_FRAMES > bench.CYCLE and (bench.RING_FRAMES - bench.CYCLE) % 96 == 0
    assert bench.CYCLE % 32 == 0
    assert bench.ring_frames(27) == 27 and [bench.ring_index(t, 27) for t in range(27)] == list(range(27))
    T = bench.ring_frames(10 * bench.RING_FRAMES)
    assert T == bench.RING_FRAMES
    idx = [bench.ring_index(t, T) for t in range(1, 5 * T)]
    assert all(0 < i < T and all(i % m == t % m for m in (bench.CYCLE, 2, 3)) for t, i in zip(range(1, 5 * T), idx))
    assert all(b == a + 1 or (a == T - 1 and b == bench.CYCLE) for a, b in zip(idx, idx[1:]))

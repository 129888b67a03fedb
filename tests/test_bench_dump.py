"""bench.py --dump-outputs: the record arrays it writes, on stand-in sessions whose fetch calls fill known records
(no device call): one float64 array per record field with a row per site, the device runs' records one after the
other, and past the size cap the same seeded sample of the sites on every run."""
import os

import numpy as np

import bench


class _Lib:
    def __init__(self, n, samples):
        self.n, self.samples = n, samples

    def ngsep_fetch_sites(self, ctx, out, cap, n_out):
        n_out._obj.value = self.n
        for i in range(min(cap, self.n) if out is not None else 0):
            out[i].pos = i + 1
            out[i].logc[9] = -0.25 * i
            out[i].strand_counts[3][1] = i
        return 0

    def ngsep_fetch_population_sites(self, ctx, sites, calls, cap, n_out):
        n_out._obj.value = self.n
        for i in range(min(cap, self.n) if sites is not None else 0):
            sites[i].pos = i + 1
            for j in range(self.samples):
                calls[i * self.samples + j].dp = 1000 * i + j
        return 0


class _Session:
    def __init__(self, n, samples=0):
        self._lib, self._ctx, self.samples = _Lib(n, samples), None, ["s"] * samples

    def _check(self, rc):
        assert rc == 0


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_single_sample_fields(tmp_path):
    bench.dump_outputs([_Session(700), _Session(0), _Session(300)], False, str(tmp_path))
    a = _load(tmp_path)
    assert "rows" not in a and "pad" not in a
    assert all(v.dtype == np.float64 and len(v) == 1000 for v in a.values())
    assert a["logc"].shape == (1000, 10) and a["strand_counts"].shape == (1000, 4, 2) and a["counts"].shape == (1000, 4)
    assert np.array_equal(a["pos"], np.concatenate([np.arange(1, 701), np.arange(1, 301)]))
    assert np.array_equal(a["logc"][:700, 9], -0.25 * np.arange(700))
    assert np.array_equal(a["strand_counts"][700:, 3, 1], np.arange(300))


def test_population_fields(tmp_path):
    bench.dump_outputs([_Session(50, samples=7)], True, str(tmp_path))
    a = _load(tmp_path)
    assert "site_pad" not in a and a["site_alleles"].shape == (50, 4)
    assert a["call_dp"].shape == (50, 7) and a["call_pl"].shape == (50, 7, 10)
    assert np.array_equal(a["call_dp"], 1000 * (a["site_pos"][:, None] - 1) + np.arange(7))


def test_sample_past_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 100_000)
    for multi, sessions in ((False, [_Session(1000)]), (True, [_Session(120, samples=7)])):
        runs = []
        for k in range(2):
            d = tmp_path / f"{int(multi)}{k}"
            bench.dump_outputs(sessions, multi, str(d))
            runs.append(_load(d))
            assert sum(v.nbytes for v in runs[-1].values()) <= 100_000
        a, b = runs
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
        rows = a["rows"]
        assert 0 < len(rows) < sessions[0]._lib.n and np.all(np.diff(rows) > 0)
        assert np.array_equal(a["site_pos" if multi else "pos"], rows + 1)
        if multi:
            assert np.array_equal(a["call_dp"][:, 3], 1000 * rows + 3)

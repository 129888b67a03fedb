"""ngsep_set_samples takes any population the reads' 16-bit sample index can carry (up to 32,767 samples): no
device is needed to describe the samples (the session is created as tests/test_capi.py::test_no_device_fails_loudly
creates one)."""
import pytest

from helpers import gpu_params
from ngsepcore_amd import GpuPileupSession, NgsepError, _lib


def _rgs(n):
    return [(f"RG{k:05d}", f"W{k:05d}") for k in range(n)]


@pytest.mark.parametrize("n", [256, 512, 4096])
def test_set_samples_beyond_255(n):
    with GpuPileupSession(gpu_params(multisample=1)) as s:
        s.set_samples(_rgs(n))
        assert len(s.samples) == n


def test_set_samples_limit_is_the_sample_index_type():
    """32,767 samples pass; one more is NGSEP_E_UNSUPPORTED with a message (include/ngsep_gpu.h)."""
    import ctypes
    with GpuPileupSession(gpu_params(multisample=1)) as s:
        for n, want in ((32767, _lib.NGSEP_OK), (32768, _lib.NGSEP_E_UNSUPPORTED)):
            ids = (ctypes.c_char_p * n)(*[b"x"] * n)
            gs = (ctypes.c_int32 * n)(*range(n))
            gr = (ctypes.c_int32 * n)()
            assert s._lib.ngsep_set_samples(s._ctx, n, ids, n, gs, gr) == want
        assert b"32767" in s._lib.ngsep_last_error(s._ctx)


def test_read_group_of_unknown_sample_is_invalid():
    """a read group mapped to sample index n_samples (one past the last) is still NGSEP_E_INVALID"""
    import ctypes
    n = 300
    with GpuPileupSession(gpu_params(multisample=1)) as s:
        ids = (ctypes.c_char_p * n)(*[f"W{k:04d}".encode() for k in range(n)])
        gs = (ctypes.c_int32 * n)(*range(n))
        gs[n - 1] = n
        gr = (ctypes.c_int32 * n)()
        with pytest.raises(NgsepError) as e:
            s._check(s._lib.ngsep_set_samples(s._ctx, n, ids, n, gs, gr))
        assert e.value.code == _lib.NGSEP_E_INVALID

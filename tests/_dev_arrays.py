"""Device arrays of one kernel call for the float64 tests (tests/test_gpu_dec_rollout_f64.py, tests/test_gpu_gru_f64.py)."""
import torch

DEV = "cuda:0"


class Arrays:
    """device arrays of one call: 16-byte aligned as torch hands them out, or every one of them 4 bytes (uint8: 1 byte) past a
    16-byte boundary -- one element more is allocated and [1:] is passed"""

    def __init__(self, unaligned):
        self.off = 1 if unaligned else 0

    def full(self, shape, value, dtype=torch.float32):
        n = 1
        for s in shape:
            n *= s
        t = torch.full((n + self.off,), value, dtype=dtype, device=DEV)[self.off:].view(*shape)
        assert t.is_contiguous() and (t.data_ptr() % 16 != 0) == bool(self.off)
        return t

    def put(self, src):
        t = self.full(tuple(src.shape), 0, src.dtype)
        t.copy_(src)
        return t

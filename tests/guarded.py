"""Guard bands for the device-entry tests (test_segment_ranges_gpu.py,
test_guard_bands_gpu.py): a tensor inside one allocation [pad | payload | pad]
whose pads must come back bit for bit.

Inputs get NaN pads: a read outside the payload that reaches a result shows as
a non-finite output. Outputs, accumulators and work buffers get the suite's
sentinel (GUARD, as in test_pwelch_batch_gpu.py): a store outside the payload
changes a pad element and the checker names it. Both pads are part of the one
allocation, so a stray access of a few rows stays in memory the test owns.

pad counts elements of the payload's type and is a multiple of 32 (256 bytes
of float64), so the payload stays 256-byte aligned like any tensor torch
allocates: alignment is not what these tests are about.
"""
import numpy as np

GUARD = -12345.0
NAN = float("nan")


def pad_for(row: int, rows: int = 2) -> int:
    """At least `rows` rows of `row` elements and 1024 elements, rounded up to
    a multiple of 32."""
    return (max(rows * int(row), 1024) + 31) // 32 * 32


def guarded(payload, fill: float, pad: int):
    """(view, check): `view` has payload's shape, type and values and lives at
    offset `pad` of one allocation of 2 * pad + payload.numel() elements on
    payload's device, every other element of which is `fill` (a complex
    element: fill in both parts). check() asserts that every pad element still
    has fill's bits (so a NaN pad can be checked too)."""
    import torch
    assert pad > 0 and pad % 32 == 0, pad
    assert payload.dtype in (torch.float64, torch.complex128), payload.dtype
    k = 2 if payload.dtype == torch.complex128 else 1
    n = payload.numel()
    base = torch.full((k * (2 * pad + n),), fill, dtype=torch.float64, device=payload.device)
    typed = torch.view_as_complex(base.view(-1, 2)) if k == 2 else base
    view = typed[pad:pad + n].view(payload.shape)
    view.copy_(payload)
    bits = base.view(torch.int64)
    want = int(np.array([fill], np.float64).view(np.int64)[0])

    def check(what: str = "guard"):
        for name, lo, hi in (("before", 0, k * pad), ("after", k * (pad + n), k * (2 * pad + n))):
            bad = torch.nonzero(bits[lo:hi] != want).flatten()
            if bad.numel():
                i = int(bad[0])
                at = (i - k * pad if name == "before" else i) // k
                raise AssertionError(
                    "%s: %d pad element(s) %s the payload changed, the first %d elements %s: %r"
                    % (what, (int(bad.numel()) + k - 1) // k, name,
                       -at if name == "before" else at,
                       "before its start" if name == "before" else "past its end",
                       float(base[lo + i])))

    return view, check

"""Shared by the three VJP test files: the accounting of a VJP reservation that grows (dmad_reserve_vjp, dmad_reserve_unet_vjp,
dmad_reserve_classifier_vjp).  Growing frees exactly what the reservation had allocated: the work maps scale with the pass size and the
packed weight images are counted once, so dmad_device_bytes rises by the same positive step from each size to the next, and a smaller
request leaves it alone.  Allocations only: no network evaluation."""


def grow(eng, reserve, sizes, got):
    """reserve(n) for each n of sizes; appends dmad_device_bytes after each call to got."""
    for n in sizes:
        reserve(n)
        got.append(eng.device_bytes())
    return got


def check(eng, reserve, got):
    """got: the figures grow() recorded for consecutive pass sizes (1, 2, 3, ...) on a fresh engine."""
    steps = [b - a for a, b in zip(got, got[1:])]
    assert len(steps) >= 2 and steps[0] > 0 and all(s == steps[0] for s in steps), got
    reserve(1)
    assert eng.device_bytes() == got[-1], (eng.device_bytes(), got)

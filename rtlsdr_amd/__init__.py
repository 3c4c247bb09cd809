"""rtlsdr_amd — MI355X (gfx950) implementation of rtl_fm's demod hot path.

The product is the C-ABI shared library built from ``rtlsdr_amd/csrc`` (see
``include/rtlfm_hip.h``).  The Python in this package is the host-side mirror
of the reference's per-buffer interface (``rtlsdr_callback`` -> ``full_demod``
-> output) over that ABI, plus build and synthetic-signal helpers.
"""
from . import capi  # noqa: F401



def channel_lowpass(ntaps: int, cutoff: float, D: int):
    """``(taps, shift)`` of rtlfm_channel_lowpass: a channel filter for ``GpuDemod.set_channel_filter`` (demod.py)."""
    from .demod import channel_lowpass as make
    return make(ntaps, cutoff, D)


def channel_bank_check(K: int, taps, shift: int) -> int:
    """rtlfm_channel_bank_check for ``GpuDemod.set_channel_bank`` (demod.py): 0 or a negative errno."""
    from .demod import channel_bank_check as chk
    return chk(K, taps, shift)


__all__ = ["capi", "channel_lowpass", "channel_bank_check"]
__version__ = "0.1.0"

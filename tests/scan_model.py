"""The scanner's model (pure Python around the oracle), for tests/test_scan_*.py.

The model is the reference's own rule around the oracle: a stream's buffers go through ``oracle.pyoracle.run_stream`` one by
one (the input with the muted bytes set to 127, rtlsdr_callback, src/rtl_fm.c:1289-1296), after every buffer the demod
thread's rule (demod_thread_fn, :1366-1370) is applied to ``state.squelch_hits``, and the emitted buffers' results are
concatenated - what the reference's output thread would have written.  ``EngineModel`` restates the hop engine of
include/rtlfm_scan.h: at most one hop per stream and run, settle, the mute of DEFAULT_BUFFER_DUMP bytes (:1504-1507).
"""
from __future__ import annotations

import copy

import numpy as np

GATE_DTYPE = [("hits_after", "<i4"), ("emit", "u1"), ("pad", "u1", (3,))]
DEFAULT_DUMP = 4096


def apply_mute(buf: np.ndarray, left: int):
    """rtlsdr_callback's mute: the first min(left, len) bytes of the buffer read 127; returns (buffer, what is left)."""
    m = min(left, buf.size)
    if m:
        buf = buf.copy()
        buf[:m] = 127
    return buf, left - m


class StreamModel:
    """One stream: carried oracle state, the pending mute, the gate."""

    def __init__(self, po, cfg, conseq: int):
        self.po, self.cfg, self.conseq = po, cfg, conseq
        self.state = po.new_states(1)[0]
        self.mute = 0

    def run(self, buffers):
        """One run: ``buffers`` = the stream's uint8 buffers in order (each its own length).  Returns (pcm int16, records)."""
        out, recs = [], np.zeros(len(buffers), dtype=GATE_DTYPE)
        for b, buf in enumerate(buffers):
            buf, self.mute = apply_mute(np.asarray(buf, dtype=np.uint8), self.mute)
            cfg = self.cfg
            if buf.size != cfg.block_len:
                cfg = copy.copy(self.cfg)
                cfg.block_len = buf.size
            pcm, self.state = self.po.run_stream(cfg, buf, self.state)
            emit = 1
            if self.state.squelch_hits > self.conseq:      # src/rtl_fm.c:1366
                self.state.squelch_hits = self.conseq + 1  # :1368
                emit = 0
            else:
                out.append(pcm)
            recs[b] = (self.state.squelch_hits, emit, 0)
        return (np.concatenate(out) if out else np.zeros(0, dtype=np.int16)), recs


class EngineModel:
    """rtlfm_scan_* for one stream, fed run by run with gate records."""

    def __init__(self, stream: int, freqs, settle: int = 0):
        self.stream, self.freqs, self.settle = stream, list(freqs), settle
        self.now = self.hold = self.serial = self.hops = self.held = 0
        self.events = []

    def feed(self, recs) -> bool:
        """Returns True when the stream hopped (its next bytes are to be muted)."""
        asked = -1
        for r in recs:
            serial = self.serial
            self.serial += 1
            if not r["emit"]:
                self.held += 1
            if self.hold > 0:
                self.hold -= 1
                continue
            if not r["emit"] and asked < 0:
                asked = serial
        if asked < 0 or len(self.freqs) <= 1:
            return False
        old = self.now
        self.now = (self.now + 1) % len(self.freqs)
        self.hops += 1
        self.hold = self.settle
        self.events.append({"stream": self.stream, "from_index": old, "to_index": self.now, "freq": self.freqs[self.now],
                            "buffer_serial": asked})
        return True

    def state(self) -> dict:
        return {"freq": self.freqs[self.now] if self.freqs else 0, "index": self.now, "hops": self.hops, "buffers": self.serial,
                "held": self.held}


def tone_or_noise(rng, nbytes: int, loud: bool) -> np.ndarray:
    """A buffer of interleaved u8 I, Q: a tone of amplitude about 100 around 127, or +-1 noise around 127."""
    n = nbytes // 2
    if loud:
        # a quarter of the sample rate up, where rtl_fm tunes its signal (the chain rotates by -90 degrees first), + a little
        ph = 2 * np.pi * (0.254 * np.arange(n) + rng.random())
        iq = np.stack([127.4 + 100.0 * np.cos(ph), 127.4 + 100.0 * np.sin(ph)], axis=1)
        return np.clip(np.rint(iq), 0, 255).astype(np.uint8).ravel()
    return (127 + rng.integers(-1, 2, nbytes)).astype(np.uint8)

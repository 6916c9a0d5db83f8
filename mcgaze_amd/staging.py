"""Between host and device memory for a DevicePipeline: the upload stages its entry points share -- pinned host buffers with device twins, used
in turn, ONE copy per call on a stream of its own --, the scope every device call of the pipeline runs in (``_call_scope``: the device, the
caller's stream, the one upload, and the mark that keeps the stage from being overwritten while the call's kernels read it), the way back for
a table the host has to read (``_host_array``) and the check of a host frame that goes up (``_bgr_frame``)."""
import sys

import numpy as np
import torch


def _host_array(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _bgr_frame(k, a):
    """Host frame ``k`` must be an HxWx3 uint8 array (TypeError) -> the array."""
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.size == 0:
        raise TypeError(f'frame {k}: frames must be HxWx3 uint8 arrays, got {a.dtype} {a.shape}')
    return a


def _layout(sizes, align=256):
    """Byte ranges of the given sizes laid out one behind the other, each starting on a multiple of ``align`` -> (offsets, total)."""
    offs = np.cumsum([0] + [(int(size) + align - 1) // align * align for size in sizes]).tolist()
    return offs[:-1], offs[-1]


class _Stage:
    """One upload stage: a pinned host buffer (``host``: its numpy view), its device twin (``base``: its address), the event of the copy between
    them (on the copy stream) and the event of the pixel kernels that read the device twin (on the caller's stream).  ``send`` copies the first
    nbytes across on the copy stream and lets the caller's stream wait for them; ``read_by`` marks the kernels launched on ``main`` as the readers."""
    pin = dev = host = copied = read = cs = main = None

    def send(self, nbytes):
        if self.read is not None:
            self.cs.wait_event(self.read)                         # the kernels that read this device buffer STAGES calls ago
        with torch.cuda.stream(self.cs):
            self.dev[:nbytes].copy_(self.pin[:nbytes], non_blocking=True)
        self.copied = self.cs.record_event()
        self.main.wait_event(self.copied)

    def read_by(self, main):
        self.read = main.record_event()


class _StagingRing:
    """The upload stages of a DevicePipeline, used in turn, and the copy stream of each device.  ``_call_scope.upload`` takes a stage, fills it and sends
    it; the scope marks it as read by the caller's stream when the call leaves."""

    def __init__(self, stages):
        self.stages, self.i, self.copy_stream = [_Stage() for _ in range(stages)], 0, {}

    def take(self, nbytes, dev, main):
        """The next upload stage, its buffers at least nbytes large: a pinned host buffer (a fresh ``pin_memory()`` per call costs
        milliseconds once decode threads compete for the allocator) and a device buffer that only the copy stream writes and only the
        pixel kernels read.  The upload runs on a stream of its own: on the caller's stream it would queue behind the forwards already
        launched there and the PCIe transfer would take its turn with the compute instead of running under it.  STAGES of them, used in
        turn, so that the host fills stage i while the copies and kernels of the stages before it are still queued."""
        st = self.stages[self.i]
        self.i = (self.i + 1) % len(self.stages)
        if st.copied is not None:
            st.copied.synchronize()                               # the pinned buffer is about to be overwritten
        cs = self.copy_stream.get(dev)
        if cs is None:
            cs = self.copy_stream[dev] = torch.cuda.Stream(dev)
        if st.pin is None or st.pin.numel() < nbytes or st.dev.device != dev:
            size = max(int(nbytes * 1.25), 1 << 20)
            st.pin = torch.empty(size, dtype=torch.uint8).pin_memory()
            st.dev = torch.empty(size, dtype=torch.uint8, device=dev)
            st.host, st.base = st.pin.numpy(), st.dev.data_ptr()
            st.read = None
            cs.wait_stream(main)                                  # the allocator may hand out memory that work queued on `main` still uses
        st.cs, st.main = cs, main
        return st


class _call_scope:
    """One device call of a DevicePipeline, ``with _call_scope(ring, dev, stream) as call:``.  The body runs on ``dev`` and on the caller's
    stream (``stream``: its handle, None: the current one), brings what it has on the host up with ONE ``call.upload`` and launches on
    ``call.main``.  When the body leaves -- at its end or by an early ``return`` -- the stage the upload took is marked as read by what was
    launched, so that a later call does not overwrite the staging buffer under those kernels; a body that took no stage marks none, and
    one that raises marks none either.
    Every call pays for the scope and host-bound calls are 30 - 60 us long (profiles/pipeline_calls_*.md), hence a class and not a
    generator, the upload written here and not forwarded to the ring, and no stream context where there is nothing to switch: once
    ``dev`` is the current device its current stream IS the caller's stream when no handle is given."""
    __slots__ = ('ring', 'dev', 'stream', 'main', 'stage', 'on_device', 'on_stream')

    def __init__(self, ring, dev, stream=None):
        self.ring, self.dev, self.stream, self.stage = ring, dev, stream, None

    def __enter__(self):
        self.on_device = torch.cuda.device(self.dev)
        self.on_device.__enter__()
        try:
            if self.stream is None:
                self.main, self.on_stream = torch.cuda.current_stream(self.dev), None
            else:
                self.main = torch.cuda.ExternalStream(self.stream, device=self.dev)
                self.on_stream = torch.cuda.stream(self.main)
                self.on_stream.__enter__()
        except BaseException:
            self.on_device.__exit__(*sys.exc_info())
            raise
        return self

    def upload(self, pixels, operands, pixels_staged=None):
        """Everything the call brings from the host, in ONE stage and one copy.  pixels: flat uint8 host arrays; operands: what the kernels
        read, each a device tensor, a host array (staged behind the pixels, in order) or None.  A device operand is read at its own
        address, a host operand at its staged one: -> (every pixel part in the device twin, as a view of it; the address of every operand,
        None for None).  When nothing comes from the host no stage is taken.  ``pixels_staged(addresses)`` runs once the pixels are in the
        pinned buffer and before the host operands are copied there, so it may still write into them (a frame table takes its frames'
        addresses, run_many its descriptors) and let go of the pixels' sources."""
        tables = [t.view(np.uint8).reshape(-1) for t in operands if isinstance(t, np.ndarray)]
        if not pixels and not tables:
            return [], [None if t is None else t.data_ptr() for t in operands]
        assert self.stage is None, 'one upload per call: the scope marks one stage'
        offs, total = _layout([b.size for b in pixels] + [b.size for b in tables])
        st = self.stage = self.ring.take(total, self.dev, self.main)
        at = [st.base + o for o in offs]
        for b, o in zip(pixels, offs):
            st.host[o:o + b.size] = b
        if pixels_staged is not None:
            pixels_staged(at[:len(pixels)])
        for b, o in zip(tables, offs[len(pixels):]):
            st.host[o:o + b.size] = b
        st.send(total)
        staged = iter(at[len(pixels):])
        return [st.dev[o:o + b.size] for b, o in zip(pixels, offs)], [None if t is None else t.data_ptr() if isinstance(t, torch.Tensor) else next(staged) for t in operands]

    def __exit__(self, kind, value, trace):
        try:
            if kind is None and self.stage is not None:
                self.stage.read_by(self.main)
        finally:
            try:
                if self.on_stream is not None:
                    self.on_stream.__exit__(kind, value, trace)
            finally:
                self.on_device.__exit__(kind, value, trace)

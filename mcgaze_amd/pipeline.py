"""Test-time data pipeline behind the reference's config surface.

``cfg.data.test.pipeline`` of the reference (configs/_base_/datasets/gaze360.py:27-36 and the L2CS variant
configs/multiclue_gaze/multiclue_gaze_r50_l2cs.py:31-39) is a list of transform dicts that mmdet's ``Compose``
(mmdet/datasets/pipelines/compose.py) runs one frame at a time on the CPU.  Here the same dicts build the same-named classes
from a ``PIPELINES`` registry, but the classes only carry the validated options and the GEOMETRY of their transform (crop
window, resized size, padded size, meta keys, and the RNG draws the reference makes, in the reference's order).  The pixel
work of the whole chain runs as ONE HIP launch per clip batch (``mcg_preprocess_frames``): decoded uint8 BGR frames go to the
device as they are, and the kernel writes the model's ``img`` tensor.  There is no CPU pixel path: without the library
``DevicePipeline.__call__`` raises.

    pipe = DevicePipeline(cfg.data.test.pipeline)
    img, img_metas = pipe(frames, device='cuda:0')            # frames: list of HxWx3 uint8 BGR arrays or file names
    model(img=[img], img_metas=[img_metas], return_loss=False, rescale=True, clip_length=7)

Head crops (``DevicePipeline.head_crops``): the demo of the reference (MCGaze_demo/demo.ipynb, cell 4) cuts one window per person out of
every video frame before this chain; there the WINDOW is chosen on the device as well (``mcg_preprocess_head_crops``), from frames and head
boxes that may both live in device memory already.  ``head_crop_window`` is the same arithmetic on the host, for checks and for drawing.
With ``pixel_format='nv12'`` the frames are a video decoder's NV12 surfaces, converted tap by tap inside the pixel kernel
(``mcg_preprocess_head_crops_nv12``); ``nv12_to_bgr`` is that conversion on the host.  The head boxes themselves can come from the raw output
of the demo's head detector without leaving the device (``DevicePipeline.detect_heads``, ``mcg_detect_heads``: confidence filter, NMS and
scale-back); ``detect_heads_host`` is the same in numpy.

Randomness: the reference's ``CenterCrop(crop_type='relative_range')`` draws the crop size from the global numpy RNG at TEST
time too (transforms.py:1126-1130), and ``RandomFlip(flip_ratio=0.0)`` consumes one more uniform
(np.random.choice, transforms.py:463-497).  ``rng`` (default: the global ``np.random``) is drawn from in that order per frame,
so a seeded single-threaded run reproduces the reference's windows; ``crop_u=<float>`` pins the draw instead.
"""
import collections
import concurrent.futures
import ctypes as C
import os
import struct
import threading
import time

import numpy as np
import torch

from . import lib as L
from .registry import Registry

PIPELINES = Registry('pipeline')


class FramePlan:
    """Geometry of one frame on its way through the chain (what the reference keeps in the ``results`` dict)."""

    def __init__(self, shape, filename=None, ori_filename=None):
        self.ori_shape = tuple(shape)
        self.filename, self.ori_filename = filename, ori_filename
        self.crop = (0, 0, shape[0], shape[1])      # y, x, h, w inside the decoded frame
        self.img_shape = tuple(shape)                # current (h, w, c)
        self.pad_shape = None
        self.scale_factor = None
        self.flip, self.flip_direction = False, None
        self.img_norm_cfg = None
        self.resized = False


@PIPELINES.register_module()
class LoadImageFromFile:
    """loading.py:36-82.  Decode happens on the host (PIL); the array stays uint8 BGR like cv2.imread's."""

    def __init__(self, to_float32=False, color_type='color', channel_order='bgr', file_client_args=dict(backend='disk')):
        if to_float32 or color_type != 'color' or channel_order != 'bgr' or file_client_args.get('backend', 'disk') != 'disk':
            raise NotImplementedError('LoadImageFromFile: only uint8 colour BGR frames from disk feed the device pipeline')

    @staticmethod
    def load(filename, rgb=False):
        """-> HxWx3 uint8, BGR like cv2.imread's (rgb=True: the decoder's RGB order as it is -- the pixel kernel swaps channels
        either way, and the per-frame flip copy is saved)."""
        from PIL import Image
        with Image.open(filename) as im:
            arr = np.asarray(im.convert('RGB'))
        return arr if rgb else np.ascontiguousarray(arr[..., ::-1])

    def plan(self, p, rng):
        pass


class _DecodeProcs:
    """``n`` decode helper processes (mcgaze_amd/_decode_worker.py) driven through a MAILBOX in shared memory: a control file next to
    the pixel ring holds one request queue per helper (fixed-size records: ring slot + path; ``head`` advanced by this side, ``tail`` by the
    helper) and one status word per ring slot (0 = being decoded, 1 = done with h, w; 2 = does not fit a slot; 3 = failed, message in the
    slot).  Nobody sleeps in a system call the other side has to wake: the helpers poll their queue (200 us naps when idle), the
    consumer polls the status word of the frame it needs.  Round 4 measured the pipe protocol this replaces at 220 us per ``write`` on
    the GPU box -- a virtual machine, where waking a task on another vCPU is an inter-processor interrupt through the hypervisor -- plus
    one reader thread per helper competing for the interpreter lock.  A request goes to the helper with the shortest queue."""

    REC = 1024                                                   # bytes per request record: int64 slot, int32 path length, path

    def __init__(self, n, ring_fd, slot_bytes, slots, ring, shm_dir=None):
        import mmap
        import tempfile
        import subprocess
        import sys
        self.n, self.slots, self.ring, self.slot_bytes = int(n), int(slots), ring, int(slot_bytes)
        self.R = 1 << max(int(slots) + 2, 2).bit_length()        # records per queue: more than there are slots, so a queue never overflows
        self.req_base = (64 + self.n * 128 + 4095) // 4096 * 4096
        self.stat_base = self.req_base + self.n * self.R * self.REC
        size = self.stat_base + self.slots * 16
        fd, path = tempfile.mkstemp(prefix='mcg_ctl_', dir=shm_dir)
        os.unlink(path)
        os.ftruncate(fd, size)                                   # sparse: only the records in use ever get pages
        self.map = mmap.mmap(fd, size)
        self.stat = np.frombuffer(self.map, dtype=np.int32, count=self.slots * 4, offset=self.stat_base).reshape(self.slots, 4)
        self.tails = np.frombuffer(self.map, dtype=np.int64, count=self.n * 16, offset=64).reshape(self.n, 16)[:, 8]
        self.heads = np.zeros(self.n, dtype=np.int64)
        worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), '_decode_worker.py')
        try:
            # -E -s: the helper ignores PYTHON* variables and the user site (a stray sitecustomize must not slow or break seven start-ups), but it
            # is TOLD where the parent's own PIL lives -- a Pillow reachable only through PYTHONPATH or `pip install --user` works
            import PIL
            pil_dir = os.path.dirname(os.path.dirname(os.path.abspath(PIL.__file__)))
            self.procs = [subprocess.Popen([sys.executable, '-E', '-s', worker, str(ring_fd), str(slot_bytes), str(fd), str(k), str(self.n), str(self.R), str(self.slots), pil_dir],
                                           stdin=subprocess.DEVNULL, pass_fds=(ring_fd, fd)) for k in range(self.n)]
        finally:
            os.close(fd)

    def submit(self, path, slot):
        """Queue ``path`` for decoding into ring slot ``slot``.  False: the path does not fit a record (the caller decodes in line)."""
        b = os.fsencode(path)
        if len(b) > self.REC - 12:
            return False
        k = int(np.argmin(self.heads - self.tails))
        h = int(self.heads[k])
        struct.pack_into(f'<qi{len(b)}s', self.map, self.req_base + (k * self.R + h % self.R) * self.REC, slot, len(b), b)
        self.stat[slot, 0] = 0
        self.heads[k] = h + 1
        struct.pack_into('<q', self.map, 64 + k * 128, h + 1)    # publish: the record and the status word are in place
        return True

    def wait(self, slot):
        """-> (state, h, w) of ring slot ``slot`` once its helper is done with it."""
        st = self.stat[slot]
        spins = 0
        while st[0] == 0:
            spins += 1
            if spins > 64:
                time.sleep(5e-5)
                if spins % 4096 == 0 and any(p.poll() is not None for p in self.procs):
                    raise RuntimeError('decode worker exited')
        if st[0] == 3:
            raise RuntimeError('decode worker: ' + bytes(self.ring[slot * self.slot_bytes:slot * self.slot_bytes + int(st[3])]).decode('utf-8', 'replace'))
        return int(st[0]), int(st[1]), int(st[2])

    def close(self):
        struct.pack_into('<q', self.map, 0, 1)                   # stop flag: the helpers leave their loop at the next poll
        for p in self.procs:
            try:
                p.wait(timeout=5)
            except Exception:
                p.kill()
                p.wait()                                         # reap it: no zombie behind a helper that had to be killed
        self.stat = self.tails = self.ring = None
        self.map = None


class FrameCache:
    """Decoded frames by path: each file is decoded once while it stays cached (LRU), optionally ahead of the consumer.

    The reference harness decodes a frame again for every window it belongs to (windows overlap by three frames,
    tools/test_gaze360_gaze.py:88-100).  Here a decode is shared by the windows that use the frame.  With ``workers`` > 0 a pool of
    host threads decodes what ``prefetch`` names ahead of the consumer (the reference uses seven loader threads); measured on the
    GPU box this LOSES to in-line decoding for small frames (a 360x360 JPEG decodes in 0.5 ms; the threads contend with the
    consumer for the interpreter lock and the allocator), so the default is in-line.  ``processes=True`` (round 4) decodes in ``workers``
    helper PROCESSES instead (``_decode_worker.py``, plain children started with subprocess: a process that holds a HIP context is
    not forked -- measured: forked workers made every later host -> device copy of the parent 58 ms slow -- and the caller's main
    module is not re-imported) that write the RGB pixels into a memory-mapped ring file in /dev/shm of ``capacity`` slots (``slot_bytes``
    each; a larger frame is decoded in line); the consumer gets numpy views of the ring (valid while the frame stays cached: run_many
    copies them into its pinned staging buffer at once).
    A ring view is only as good as its slot: a frame handed out as a view is therefore PINNED -- never evicted -- until ``release()``
    (run_many calls it once its staging copy is made); a call that needs more distinct frames at once than the cache has slots raises
    instead of handing out a view whose slot a later decode overwrites.  A caller that uses the cache directly calls ``release()`` when it
    is done with the views it holds.  ``processes=True`` needs (capacity + 1) * slot_bytes of /dev/shm at most (pages are touched as slots
    are used: ``frame_bytes``, the decoded size the caller expects, prices a slot in the check; a node's ranks share the tmpfs,
    LOCAL_WORLD_SIZE); when the tmpfs cannot back that (a container's default /dev/shm is 64 MB), the cache falls back to IN-LINE decoding
    with a warning -- a tmpfs that runs out under a mapped write is a SIGBUS in a helper, not an exception.
    Only the DECODE is shared: crop draws, geometry and the pixel kernel still run per window, in the caller's order -- results do
    not depend on the cache, the worker count or the worker kind."""

    def __init__(self, workers=0, capacity=512, loader=None, processes=False, slot_bytes=3 << 20, frame_bytes=None):
        self.rgb = loader is None                   # our own decode keeps the decoder's RGB order (DevicePipeline.run_many swaps in the kernel)
        self.loader = loader or (lambda path: LoadImageFromFile.load(path, rgb=True))
        self.capacity = max(int(capacity), 1)
        self.ring, self._map, self.procs, self.free, self.slot_bytes = None, None, None, [], int(slot_bytes)
        self.pool = None
        if workers > 0 and processes:
            if loader is not None:
                raise ValueError('FrameCache(processes=True) decodes with its own worker (PIL, RGB)')
            import tempfile
            # both shared files are ANONYMOUS: created in /dev/shm, unlinked at once, handed to the helpers as inherited descriptors -- nothing
            # is left behind there however this process ends
            shm = '/dev/shm' if os.path.isdir('/dev/shm') else None
            # The ring file is sparse: a slot costs the pages its frame touches.  The check prices a slot at ``frame_bytes`` -- the decoded size
            # the caller expects (harness: the first frame of the run, 390 KB for 360 x 360) -- or, unknown, at the whole slot; the tmpfs is
            # shared by the ranks of a node, so each rank may count on its share only (LOCAL_WORLD_SIZE).  
            per_slot = min(int(frame_bytes), self.slot_bytes) if frame_bytes else self.slot_bytes
            per_slot = (max(per_slot, 1) + 4095) // 4096 * 4096
            ranks = max(int(os.environ.get('LOCAL_WORLD_SIZE', '1') or 1), 1)
            try:
                vfs = os.statvfs(shm or tempfile.gettempdir())
                fit = int(vfs.f_bavail * vfs.f_frsize * 0.8 / ranks) // per_slot - 1     # slots the file system can back, with a margin
            except OSError:
                fit = self.capacity
            if fit < self.capacity + 1:                          # (no half measures -- a ring smaller than one run_many call's frames would only move the failure)
                import warnings
                warnings.warn(f'FrameCache: {shm or tempfile.gettempdir()} cannot back {self.capacity + 1} ring slots of {per_slot} bytes for each of {ranks} rank(s) '
                              f'(room for {max(fit, 0)}); decoding in line instead of in helper processes')
                processes, workers = False, 0                    # in line, not threads: decode threads LOSE to in-line decoding (class docstring)
        if workers > 0 and processes:
            fd, path = tempfile.mkstemp(prefix='mcg_ring_', dir=shm)
            os.unlink(path)
            import mmap
            try:
                os.ftruncate(fd, (self.capacity + 1) * self.slot_bytes)           # sparse: a slot gets pages when a frame is written into it
                self._map = mmap.mmap(fd, (self.capacity + 1) * self.slot_bytes)
                self.ring = np.frombuffer(self._map, dtype=np.uint8)   # a plain ndarray: np.memmap's subclass machinery cost 5 us per slice
                self.free = list(range(self.capacity + 1))
                self.procs = _DecodeProcs(int(workers), fd, self.slot_bytes, self.capacity + 1, self.ring, shm)
            finally:
                os.close(fd)
        elif workers > 0:
            self.pool = concurrent.futures.ThreadPoolExecutor(max_workers=int(workers), thread_name_prefix='mcg-decode')
        self.items = collections.OrderedDict()      # path -> Future (threads) / ring slot (processes) / array (in line), least recently used first
        self.used = collections.OrderedDict()       # paths the consumer has already asked for, oldest use first: the eviction candidates
        self.held = set()                           # paths handed out as ring views since the last release(): not evictable
        self.lock = threading.Lock()
        self.decodes = 0
        self.waits, self.wait_s, self.first_wait_s = 0, 0.0, 0.0            # times the consumer found a frame not decoded yet, and how long it then waited

    def _entry(self, path, wanted_now):
        with self.lock:
            e = self.items.get(path)
            if wanted_now:
                self.used[path] = True
                self.used.move_to_end(path)
            if e is not None:
                self.items.move_to_end(path)
                return e
            if self.pool is None and self.procs is None and not wanted_now:
                return None                         # in-line mode: prefetch is a no-op, the decode happens when the frame is asked for
            if self.procs is not None:
                while len(self.items) >= self.capacity:          # make room first: the new decode needs a ring slot
                    self._evict()
                slot = self.free.pop()
                if self.procs.submit(path, slot):
                    e = self.items[path] = slot
                else:                                            # a path too long for a request record: decoded here
                    self.free.append(slot)
                    e = self.items[path] = self.loader(path)
            else:
                e = self.items[path] = self.pool.submit(self.loader, path) if self.pool is not None else self.loader(path)
            self.decodes += 1
            while len(self.items) > self.capacity:
                self._evict()
            return e

    def _evict(self):
        # A frame decoded AHEAD and not yet asked for is the one the consumer needs next: plain LRU threw exactly those out (they are the
        # oldest entries once the cache is full -- every prefetch then cost a second, synchronous decode: round 3's "threads are slower").
        # Victims are frames already consumed, oldest use first; an unconsumed one only when nothing else is left.
        victim, kept = None, []
        while self.used and victim is None:
            p, _ = self.used.popitem(last=False)
            if p in self.held:
                kept.append(p)                                   # its view is still out: not a candidate (back in line below)
            elif p in self.items:
                victim = p
        for p in reversed(kept):
            self.used[p] = True
            self.used.move_to_end(p, last=False)
        if victim is None:
            victim = next((p for p in self.items if p not in self.held), None)
            if victim is None:
                raise RuntimeError(f'FrameCache: all {len(self.items)} cached frames are handed out as views of the decode ring; raise capacity '
                                   f'({self.capacity}) above the distinct frames of one run_many call, or release() between uses')
        old = self.items.pop(victim)
        if isinstance(old, int):                                 # ring slot: its writer must be done before the slot is handed out again
            try:
                self.procs.wait(old)
            except RuntimeError:
                pass
            self.free.append(old)

    def prefetch(self, paths):
        """Start decoding ``paths`` ahead of their use (a no-op for in-line decoding)."""
        if self.pool is not None or self.procs is not None:
            for p in paths:
                self._entry(p, False)

    def _wait(self, e):
        """The decode behind entry ``e`` (a Future of the thread pool or a ring slot of the helper processes), counting the times the
        consumer had to wait for it."""
        if isinstance(e, int):
            if self.procs.stat[e, 0] != 0:
                return self.procs.wait(e)
            wait = lambda: self.procs.wait(e)
        else:
            if e.done():
                return e.result()
            wait = e.result
        t0 = time.perf_counter()
        r = wait()
        dt = time.perf_counter() - t0
        if self.waits == 0:
            self.first_wait_s = dt                               # mostly the helpers' start-up (interpreter + PIL import)
        self.waits += 1
        self.wait_s += dt
        return r

    def __call__(self, path):
        e = self.items.get(path)
        if e is None:
            e = self._entry(path, True)
        else:                                                    # the common case (decoded ahead), without _entry's bookkeeping
            self.used[path] = True
            self.used.move_to_end(path)
        if isinstance(e, int):                                   # decoded by a helper process into ring slot e
            state, h, w = self._wait(e)
            if state == 2:
                return self.loader(path)                         # larger than a slot: decoded here
            o = e * self.slot_bytes
            with self.lock:
                self.held.add(path)                              # a view of the ring: the slot stays until release()
            return self.ring[o:o + h * w * 3].reshape(h, w, 3)
        return self._wait(e) if isinstance(e, concurrent.futures.Future) else e

    def release(self):
        """The views handed out so far are no longer read (run_many: copied into the staging buffer): their slots may be evicted again."""
        with self.lock:
            self.held.clear()

    def close(self):
        if self.pool is not None:
            self.pool.shutdown(wait=False, cancel_futures=True)
        if self.procs is not None:
            self.procs.close()
            self.procs = None
        self.items.clear()
        self.used.clear()
        self.ring = None                                         # (views handed out earlier keep the mapping alive; it goes with the last of them)
        self._map = None


@PIPELINES.register_module()
class CenterCrop:
    """transforms.py:953-1160: a CENTRED window whose size follows ``crop_type`` (the random offsets are commented out
    upstream, :1040-1043); 'relative_range' draws ONE uniform for both sides (:1126-1130)."""

    def __init__(self, crop_size, crop_type='absolute', allow_negative_crop=False, recompute_bbox=False, bbox_clip_border=True, crop_u=None):
        if crop_type not in ['relative_range', 'relative', 'absolute', 'absolute_range']:
            raise ValueError(f'Invalid crop_type {crop_type}.')
        if crop_type in ['absolute', 'absolute_range']:
            assert crop_size[0] > 0 and crop_size[1] > 0
            assert isinstance(crop_size[0], int) and isinstance(crop_size[1], int)
        else:
            assert 0 < crop_size[0] <= 1 and 0 < crop_size[1] <= 1
        self.crop_size, self.crop_type, self.crop_u = crop_size, crop_type, crop_u
        if crop_type == 'relative_range':
            # upstream: cs = float32 array, u = float64 array -> cs + u * (1 - cs) with (1 - cs) rounded in f32 and the rest in f64.
            # The same values as python floats (one rounding per operation, like the array expression), without three array temporaries per frame.
            cs = np.asarray(crop_size, dtype=np.float32)
            self._cs = [float(v) for v in cs]
            self._rest = [float(v) for v in (1 - cs)]

    def _get_crop_size(self, h, w, rng):
        if self.crop_type == 'absolute':
            return min(self.crop_size[0], h), min(self.crop_size[1], w)
        if self.crop_type == 'absolute_range':
            assert self.crop_size[0] <= self.crop_size[1]
            crop_h = rng.randint(min(h, self.crop_size[0]), min(h, self.crop_size[1]) + 1)
            crop_w = rng.randint(min(w, self.crop_size[0]), min(w, self.crop_size[1]) + 1)
            return crop_h, crop_w
        if self.crop_type == 'relative':
            return int(h * self.crop_size[0] + 0.5), int(w * self.crop_size[1] + 0.5)
        u = rng.random_sample() if self.crop_u is None else float(self.crop_u)        # ONE uniform for both sides (:1126-1130; rand(1) draws the same double)
        crop_h, crop_w = self._cs[0] + u * self._rest[0], self._cs[1] + u * self._rest[1]
        return int(h * crop_h + 0.5), int(w * crop_w + 0.5)

    def plan(self, p, rng):
        if p.resized:
            raise NotImplementedError('CenterCrop after Resize is not a chain the device kernel fuses')
        y, x, h, w = p.crop
        ch, cw = self._get_crop_size(h, w, rng)
        assert ch > 0 and cw > 0
        oy, ox = int(max(h - ch, 0) / 2 + 0.5), int(max(w - cw, 0) / 2 + 0.5)
        ch, cw = min(ch, h - oy), min(cw, w - ox)
        p.crop = (y + oy, x + ox, ch, cw)
        p.img_shape = (ch, cw) + p.img_shape[2:]


@PIPELINES.register_module()
class Resize:
    """transforms.py:31-330 for the single-scale test-time use: keep_ratio -> mmcv.imrescale's size rule, else exact size;
    bilinear (cv2.INTER_LINEAR), which is what the kernel implements."""

    def __init__(self, img_scale=None, multiscale_mode='range', ratio_range=None, keep_ratio=True, bbox_clip_border=True, backend='cv2',
                 override=False, interpolation='bilinear'):
        if isinstance(img_scale, list):
            if len(img_scale) != 1:
                raise NotImplementedError('Resize: multi-scale sampling is a training option')
            img_scale = img_scale[0]
        if img_scale is None or ratio_range is not None or backend != 'cv2' or interpolation != 'bilinear':
            raise NotImplementedError('Resize: only img_scale=(w, h) with the cv2 bilinear backend is supported')
        assert isinstance(img_scale, tuple) and len(img_scale) == 2
        self.img_scale, self.keep_ratio = img_scale, keep_ratio

    def plan(self, p, rng):
        if p.resized:
            raise NotImplementedError('two Resize transforms in one pipeline')
        h, w = p.img_shape[:2]
        if self.keep_ratio:
            f = min(max(self.img_scale) / max(h, w), min(self.img_scale) / min(h, w))
            new_w, new_h = int(w * float(f) + 0.5), int(h * float(f) + 0.5)
        else:
            new_w, new_h = self.img_scale
        p.scale_factor = np.array([new_w / w, new_h / h, new_w / w, new_h / h], dtype=np.float32)
        p.img_shape = (new_h, new_w) + p.img_shape[2:]
        p.pad_shape = p.img_shape
        p.resized = True


@PIPELINES.register_module()
class RandomFlip:
    """transforms.py:333-530.  Only the never-flipping test-time setting is supported; it still consumes the uniform
    np.random.choice draws in the reference (:485)."""

    def __init__(self, flip_ratio=None, direction='horizontal'):
        if isinstance(flip_ratio, list) or direction != 'horizontal':
            raise NotImplementedError('RandomFlip: list ratios / non-horizontal directions are training options')
        if isinstance(flip_ratio, float):
            assert 0 <= flip_ratio <= 1
        elif flip_ratio is not None:
            raise ValueError('flip_ratios must be None, float, or list of float')
        if flip_ratio:
            raise NotImplementedError('RandomFlip: flip_ratio > 0 is a training option; the test pipeline uses 0.0')
        self.flip_ratio = flip_ratio

    def plan(self, p, rng):
        if self.flip_ratio is not None:
            rng.random_sample()
        p.flip, p.flip_direction = False, None


@PIPELINES.register_module()
class Normalize:
    """transforms.py:722-760."""

    def __init__(self, mean, std, to_rgb=True):
        self.mean, self.std, self.to_rgb = np.array(mean, dtype=np.float32), np.array(std, dtype=np.float32), to_rgb
        self._cfg = dict(mean=self.mean, std=self.std, to_rgb=self.to_rgb)       # one object for every frame's meta (read-only by convention)

    def plan(self, p, rng):
        p.img_norm_cfg = self._cfg


@PIPELINES.register_module()
class Pad:
    """transforms.py:623-720: zeros below / right, up to a multiple of size_divisor or a fixed size."""

    def __init__(self, size=None, size_divisor=None, pad_to_square=False, pad_val=dict(img=0, masks=0, seg=255)):
        if pad_to_square:
            raise NotImplementedError('Pad: pad_to_square')
        assert size is not None or size_divisor is not None, 'only one of size and size_divisor should be valid'
        assert size is None or size_divisor is None
        v = pad_val.get('img', 0) if isinstance(pad_val, dict) else pad_val
        if v != 0:
            raise NotImplementedError('Pad: the device kernel pads with zeros')
        self.size, self.size_divisor = size, size_divisor

    def plan(self, p, rng):
        h, w = p.img_shape[:2]
        if self.size is not None:
            ph, pw = max(self.size[0], h), max(self.size[1], w)
        else:
            d = self.size_divisor
            ph, pw = -(-h // d) * d, -(-w // d) * d                      # int(np.ceil(h / d)) * d
        p.pad_shape = (ph, pw) + p.img_shape[2:]


@PIPELINES.register_module()
class DefaultFormatBundle:
    """formatting.py:175-260: HWC -> CHW tensor; the kernel writes that layout."""

    def __init__(self, img_to_float=True, pad_val=dict(img=0, masks=0, seg=255)):
        pass

    def plan(self, p, rng):
        if p.pad_shape is None:
            p.pad_shape = p.img_shape
        if p.scale_factor is None:
            p.scale_factor = 1.0


@PIPELINES.register_module()
class ImageToTensor:
    def __init__(self, keys):
        self.keys = keys

    def plan(self, p, rng):
        pass


@PIPELINES.register_module()
class Collect:
    """formatting.py:279-352."""

    def __init__(self, keys, meta_keys=('filename', 'ori_filename', 'ori_shape', 'img_shape', 'pad_shape', 'scale_factor', 'flip',
                                        'flip_direction', 'img_norm_cfg')):
        if list(keys) != ['img']:
            raise NotImplementedError(f'Collect: the test pipeline collects only img (got {keys})')
        self.keys, self.meta_keys = keys, meta_keys

    def plan(self, p, rng):
        pass

    def meta(self, p):
        return {k: getattr(p, k) for k in self.meta_keys}


_DESC = np.dtype([('src', np.uint64)] + [(f, np.int32) for f in ('src_h', 'src_w', 'src_pitch', 'crop_y', 'crop_x', 'crop_h', 'crop_w', 'out_h', 'out_w')],
                 align=True)                       # lib.FrameDesc / mcg_frame_desc, as a numpy record
assert _DESC.itemsize == C.sizeof(L.FrameDesc) and all(_DESC.fields[n][1] == getattr(L.FrameDesc, n).offset for n in _DESC.names)


_IMAGE = np.dtype([('src', np.uint64), ('h', np.int32), ('w', np.int32), ('pitch', np.int32)], align=True)   # lib.ImageDesc / mcg_image_desc
assert _IMAGE.itemsize == C.sizeof(L.ImageDesc) and all(_IMAGE.fields[n][1] == getattr(L.ImageDesc, n).offset for n in _IMAGE.names)
_DESC_WORDS = _DESC.itemsize // 4
# the NV12 records: lib.Nv12ImageDesc / mcg_nv12_image_desc, and mcg_nv12_frame_desc = the fields of _DESC, then the UV plane and its pitch
_NV12_IMAGE = np.dtype([('y', np.uint64), ('uv', np.uint64), ('h', np.int32), ('w', np.int32), ('pitch_y', np.int32), ('pitch_uv', np.int32)], align=True)
assert _NV12_IMAGE.itemsize == C.sizeof(L.Nv12ImageDesc) and all(_NV12_IMAGE.fields[n][1] == getattr(L.Nv12ImageDesc, n).offset for n in _NV12_IMAGE.names)
_NV12_DESC = np.dtype([(n, _DESC.fields[n][0]) for n in _DESC.names] + [('uv', np.uint64), ('uv_pitch', np.int32)], align=True)
assert _NV12_DESC.itemsize == C.sizeof(L.Nv12FrameDesc) and all(_NV12_DESC.fields[n][1] == getattr(L.Nv12FrameDesc, n).offset for n in _NV12_DESC.names)
_NV12_DESC_WORDS = _NV12_DESC.itemsize // 4
_CROP_WORD = _DESC.fields['crop_y'][1] // 4         # crop_y, crop_x, crop_h, crop_w are consecutive int32 words of a descriptor


# YUV -> RGB coefficients at 20 fractional bits (include/mcgaze_hip.h, mcg_yuv_coef).  bt601: OpenCV's published limited-range constants
# (its ITUR_BT_601_* set, 1.164 / 2.018 / -0.391 / -0.813 / 1.596 scaled by 2^20), restated, not linked: parity with cv2's COLOR_YUV2BGR_NV12
# is not pinned on any machine this was built on.  bt709: limited range, round(c * 2**20) of the matrix with Kr = 0.2126, Kb = 0.0722,
# luma scale 255/219 and chroma scale 255/224, worked out once in double: cy = 255/219, cub = 2 (1 - Kb) 255/224,
# cug = -(Kb / Kg) 2 (1 - Kb) 255/224, cvg = -(Kr / Kg) 2 (1 - Kr) 255/224, cvr = 2 (1 - Kr) 255/224 with Kg = 1 - Kr - Kb.
YUV_COEF = {
    'bt601': dict(y_off=16, cy=1220542, cub=2116026, cug=-409993, cvg=-852492, cvr=1673527),
    'bt709': dict(y_off=16, cy=1220945, cub=2215014, cug=-223607, cvg=-558796, cvr=1879825),
}


def _yuv_coef(matrix):
    if matrix not in YUV_COEF:
        raise ValueError(f'matrix must be one of {sorted(YUV_COEF)}, got {matrix!r}')
    return YUV_COEF[matrix]


def _nv12_planes(k, im, dev=None):
    """One NV12 surface as head_crops takes it -> (y [H,W], uv [H/2,W] as a 2-d view, on_device): a (y, uv) pair with uv [H/2,W/2,2] or
    [H/2,W], or a single [3H/2, W] surface (Y rows, then the UV rows).  TypeError for a wrong dtype, rank or device, ValueError for odd sizes
    or a UV plane that does not belong to the Y plane."""
    if isinstance(im, (tuple, list)):
        if len(im) != 2:
            raise TypeError(f'frame {k}: an NV12 frame is a (y, uv) pair or one [3H/2, W] surface, got a sequence of {len(im)}')
        y, uv = im
    else:
        y, uv = im, None
    on_device = isinstance(y, torch.Tensor)
    if uv is not None and isinstance(uv, torch.Tensor) != on_device:
        raise TypeError(f'frame {k}: the Y and UV planes must both be numpy arrays or both be device tensors')
    if not on_device:
        y = np.asarray(y)
        uv = None if uv is None else np.asarray(uv)
    u8 = torch.uint8 if on_device else np.uint8
    for name, t in (('Y', y), ('UV', uv)):
        if t is None:
            continue
        if t.dtype != u8 or t.ndim not in ((2,) if name == 'Y' else (2, 3)) or (t.numel() if on_device else t.size) == 0:
            raise TypeError(f'frame {k}: the {name} plane must be a non-empty uint8 array of rank {"2" if name == "Y" else "2 or 3"}, got {t.dtype} {tuple(t.shape)}')
        if on_device and not (t.is_cuda and t.device == dev):
            raise TypeError(f'frame {k}: device planes must be uint8 tensors on {dev}, got one on {t.device}')
    if uv is None:                                                # one surface: 3H/2 rows
        rows, w = y.shape
        if rows % 3 or w % 2:
            raise ValueError(f'frame {k}: a {rows} x {w} surface is not [3H/2, W] with H and W even')
        h = rows // 3 * 2
        y, uv = y[:h], y[h:]
    h, w = y.shape
    if h % 2 or w % 2:
        raise ValueError(f'frame {k}: NV12 frames have even sizes, got {h} x {w}')
    if tuple(uv.shape) not in ((h // 2, w // 2, 2), (h // 2, w)):
        raise ValueError(f'frame {k}: the UV plane of a {h} x {w} frame is [{h // 2}, {w // 2}, 2] or [{h // 2}, {w}], got {tuple(uv.shape)}')
    if on_device:
        # rows may lie further apart than w bytes (a decoder's pitch); inside a row the bytes are packed
        packed = y.stride(1) == 1 and (uv.stride(1) == 1 if uv.ndim == 2 else (uv.stride(2) == 1 and (uv.shape[1] == 1 or uv.stride(1) == 2)))
        if not (packed and y.stride(0) >= w and (uv.shape[0] == 1 or uv.stride(0) >= w)):
            raise TypeError(f'frame {k}: device planes must have packed rows at least {w} bytes apart, got strides {tuple(y.stride())} and {tuple(uv.stride())}')
        if uv.ndim == 3:
            uv = uv.as_strided((h // 2, w), (uv.stride(0), 1))
    else:
        y, uv = np.ascontiguousarray(y), np.ascontiguousarray(uv).reshape(h // 2, w)
    return y, uv, on_device


def nv12_to_bgr(y, uv, matrix='bt601'):
    """An NV12 frame -> HxWx3 uint8 BGR on the host, in the arithmetic the pixel kernel applies per tap (csrc/preprocess.hip, Nv12Source):
    y [H,W] uint8, uv [H/2,W/2,2] or [H/2,W] uint8 interleaved (U, V), H and W even; matrix: a key of YUV_COEF.  Chroma is the nearest
    sample, uv[y >> 1][x >> 1], and with u = U - 128, v = V - 128 in 32-bit integers (>> is an arithmetic shift):

        yy = max(0, Y - y_off) * cy
        R = sat8((yy + cvr * v + (1 << 19)) >> 20);  G = sat8((yy + cvg * v + cug * u + (1 << 19)) >> 20);  B = sat8((yy + cub * u + (1 << 19)) >> 20)

    head_crops(pixel_format='nv12') on the planes equals head_crops on this frame bit for bit."""
    k = _yuv_coef(matrix)
    y, uv, _ = _nv12_planes(0, (np.asarray(y), np.asarray(uv)))
    h, w = y.shape
    c = uv.reshape(h // 2, w // 2, 2).astype(np.int32) - 128
    u, v = (np.repeat(np.repeat(c[..., j], 2, axis=0), 2, axis=1) for j in (0, 1))
    yy = np.maximum(0, y.astype(np.int32) - k['y_off']) * np.int32(k['cy']) + np.int32(1 << 19)
    sat8 = lambda t: np.clip(t >> 20, 0, 255).astype(np.uint8)
    return np.stack([sat8(yy + k['cub'] * u), sat8(yy + k['cvg'] * v + k['cug'] * u), sat8(yy + k['cvr'] * v)], axis=-1)


def _yuv_to_bgr(yuv, k):
    """(Y, U, V) integer arrays [..., 3] -> BGR [..., 3] int32 by nv12_to_bgr's arithmetic."""
    yuv = np.asarray(yuv, dtype=np.int32)
    u, v = yuv[..., 1] - 128, yuv[..., 2] - 128
    yy = np.maximum(0, yuv[..., 0] - k['y_off']) * np.int32(k['cy']) + np.int32(1 << 19)
    sat8 = lambda t: np.clip(t >> 20, 0, 255)
    return np.stack([sat8(yy + k['cub'] * u), sat8(yy + k['cvg'] * v + k['cug'] * u), sat8(yy + k['cvr'] * v)], axis=-1)


def bgr_to_yuv(color, matrix='bt601'):
    """The (Y, U, V) an NV12 surface is drawn with so that it SHOWS the BGR colour ``color`` -> uint8 [3].  No new constants: the matrix of
    ``YUV_COEF[matrix]`` (B = cy y + cub u, G = cy y + cug u + cvg v, R = cy y + cvr v with y = Y - y_off, u = U - 128, v = V - 128, each
    coefficient / 2^20) is inverted numerically and the result rounded; among the triples within 2 of it in every component (and inside
    [0, 255]) the one whose conversion by nv12_to_bgr's integer arithmetic has the smallest maximum channel error against ``color`` is taken,
    ties going to the smallest (Y, U, V) in lexicographic order.  Runs once per colour, on the host."""
    k = _yuv_coef(matrix)
    c = np.asarray(color)
    if c.shape != (3,) or c.dtype.kind not in 'iu' or c.min() < 0 or c.max() > 255:
        raise ValueError(f'a colour is three integers in [0, 255] (B, G, R), got {color!r}')
    c = c.astype(np.int64)
    m = np.array([[k['cy'], k['cub'], 0], [k['cy'], k['cug'], k['cvg']], [k['cy'], 0, k['cvr']]], dtype=np.float64) / float(1 << 20)
    centre = np.rint(np.linalg.solve(m, c.astype(np.float64)) + np.array([k['y_off'], 128.0, 128.0])).astype(np.int64)
    grid = np.stack(np.meshgrid(*[np.arange(v - 2, v + 3) for v in centre], indexing='ij'), axis=-1).reshape(-1, 3)     # lexicographic order
    grid = grid[((grid >= 0) & (grid <= 255)).all(axis=1)]
    if not len(grid):                                            # (cannot happen for a colour in [0, 255]^3: its YUV is inside the nominal range)
        raise ValueError(f'no (Y, U, V) near {centre.tolist()} for colour {color!r}')
    err = np.abs(_yuv_to_bgr(grid, k) - c).max(axis=1)
    return grid[int(np.argmin(err))].astype(np.uint8)            # argmin: the FIRST of the smallest, i.e. the lexicographically smallest


ARROW_COLOR = (230, 253, 11)                                     # the demo's, BGR (MCGaze_demo/demo.ipynb, cell 5)
ARROW_COORD, ARROW_SIDE = 8191, 8192                             # the bound under which the coverage test is exact in 64-bit integers
_ARROW = np.dtype([('seg', np.int32, (3, 2, 2)), ('thickness', np.int32)] + [(f, np.int32) for f in ('x0', 'y0', 'x1', 'y1', 'image', 'flag', 'reserved')])
assert _ARROW.itemsize == C.sizeof(L.ArrowDesc) and all(_ARROW.fields[n][1] == getattr(L.ArrowDesc, n).offset for n in _ARROW.names)
_ARROW_WORDS = _ARROW.itemsize // 4


def _arrow_params(length=1.0, min_thickness=5, thickness_ratio=0.01, tip_length=0.1):
    """The arrow parameters, validated (ValueError) -> (length, min_thickness, thickness_ratio, tip_length); the defaults are the demo's."""
    length, thickness_ratio, tip_length = float(length), float(thickness_ratio), float(tip_length)
    if not all(np.isfinite(v) for v in (length, thickness_ratio, tip_length)):
        raise ValueError('length, thickness_ratio and tip_length must be finite')
    if int(min_thickness) != min_thickness or not 1 <= int(min_thickness) <= 255:
        raise ValueError(f'min_thickness must be an integer in 1 .. 255, got {min_thickness!r}')
    return length, int(min_thickness), thickness_ratio, tip_length


def arrow_segments(boxes, gaze, **params):
    """The arrow plan on the host (include/mcgaze_hip.h, "annotated frames out"; arrow_plan_kernel line for line): boxes [n,4] x1 y1 x2 y2, gaze
    [n,>=2], both read as f32 and widened to double; params: length, min_thickness, thickness_ratio, tip_length (the demo's by default).
    -> (seg int64 [n,3,2,2]: shaft, stroke, stroke x (from, to) x (x, y); thickness int64 [n]; flags int32 [n]).  seg[:, 0] is
    harness.head_arrows of the same input.  Flag 2 (and a zero row): a box or gaze that is not finite, an end point outside [-8191, 8191] or a
    thickness above 255."""
    length, min_thickness, ratio, tip_length = _arrow_params(**params)
    b = np.asarray(boxes, dtype=np.float32).astype(np.float64).reshape(-1, 4)
    g = np.asarray(gaze, dtype=np.float32).astype(np.float64)
    g = g.reshape(len(b), -1)[:, :2] if g.size else np.zeros((len(b), 2 if not len(b) else 0))
    if g.shape[1] != 2:
        raise ValueError(f'gaze must be [n, >= 2], got {np.shape(gaze)}')
    ok = np.isfinite(b).all(axis=1) & np.isfinite(g).all(axis=1)
    b, g = np.where(ok[:, None], b, 0.0), np.where(ok[:, None], g, 0.0)
    inside = lambda *vs: np.logical_and.reduce([np.abs(v) <= ARROW_COORD for v in vs])
    # numpy rounds every elementwise product and sum on its own: nothing is contracted, as in the kernel
    cx, cy = np.floor(np.trunc(b[:, 0] + b[:, 2]) / 2.0), np.floor(np.trunc(b[:, 1] + b[:, 3]) / 2.0)
    l = np.trunc(np.maximum(b[:, 3] - b[:, 1], b[:, 2] - b[:, 0]) * length)
    tx, ty = np.trunc(cx - l * g[:, 0]), np.trunc(cy - l * g[:, 1])
    t = np.maximum(float(min_thickness), np.trunc(l * ratio))
    ok &= inside(cx, cy, tx, ty) & (t <= 255.0)
    cx, cy, tx, ty, t = (np.where(ok, v, 0.0) for v in (cx, cy, tx, ty, t))
    dx, dy = cx - tx, cy - ty
    k = tip_length * 0.7071067811865476
    ax, ay = np.rint(tx + k * (dx - dy)), np.rint(ty + k * (dx + dy))          # np.rint rounds half to even
    bx, by = np.rint(tx + k * (dx + dy)), np.rint(ty + k * (dy - dx))
    ok &= inside(ax, ay, bx, by)
    tip = np.stack([tx, ty], axis=1)
    seg = np.stack([np.stack([np.stack([px, py], axis=1), tip], axis=1) for px, py in ((cx, cy), (ax, ay), (bx, by))], axis=1)
    seg, t = np.where(ok[:, None, None, None], seg, 0.0), np.where(ok, t, 0.0)
    return seg.astype(np.int64), t.astype(np.int64), np.where(ok, 0, 2).astype(np.int32)


def segment_coverage(h, w, a, b, t, y0=0, x0=0):
    """bool [h,w]: which pixels (integer centres (x0 + column, y0 + row)) belong to the segment a -> b (x, y each) of thickness t, i.e. lie
    within t / 2 of it -- a capsule, a disc for a segment of no length -- exactly, in 64-bit integers (the kernel's test, include/mcgaze_hip.h)."""
    py, px = np.mgrid[y0:y0 + h, x0:x0 + w].astype(np.int64)
    ax, ay, bx, by, tt = int(a[0]), int(a[1]), int(b[0]), int(b[1]), int(t) * int(t)
    dx, dy, qx, qy = bx - ax, by - ay, px - ax, py - ay
    L, u = dx * dx + dy * dy, qx * dx + qy * dy
    qq, rr = qx * qx + qy * qy, (px - bx) ** 2 + (py - by) ** 2
    return np.where(u <= 0, 4 * qq <= tt, np.where(u >= L, 4 * rr <= tt, 4 * (qq * L - u * u) <= tt * L))


def _arrow_colors(color, n, nv12, matrix):
    """-> (one uint8 [3] or None, per-row uint8 [n,3] or None), as the entries take them: B, G, R, or with nv12 the (Y, U, V) of bgr_to_yuv."""
    c = np.asarray(ARROW_COLOR if color is None else _host_array(color))
    if c.dtype.kind not in 'iu' or c.shape not in ((3,), (n, 3)) or (c.size and (c.min() < 0 or c.max() > 255)):
        raise ValueError(f'color must be one (B, G, R) triple or one per row, [{n}, 3], integers in [0, 255]; got {c.dtype} {c.shape}')
    c = c.astype(np.uint8)
    if nv12:
        if c.ndim == 1:
            c = bgr_to_yuv(c, matrix)
        else:
            uniq, inverse = np.unique(c, axis=0, return_inverse=True)
            c = np.stack([bgr_to_yuv(v, matrix) for v in uniq]).reshape(-1, 3)[inverse.reshape(-1)] if n else c
    return (c, None) if c.ndim == 1 else (None, np.ascontiguousarray(c))


def _arrow_rows(boxes, gaze, image_of, sizes, strict, **params):
    """Plan and flags of n rows on the host -> (seg, thickness, flags): arrow_segments plus what depends on the frames -- an image_of outside
    ``sizes`` ([(h, w), ...]) and an image larger than 8192 a side are flag 2.  strict: ValueError instead, naming the first such row."""
    seg, t, flags = arrow_segments(boxes, gaze, **params)
    image_of = np.asarray(image_of).reshape(-1)
    if image_of.dtype.kind not in 'iu':
        raise TypeError(f'image_of must hold integers, got {image_of.dtype}')
    if len(image_of) != len(flags):
        raise ValueError(f'boxes {np.shape(boxes)}, gaze {np.shape(gaze)} and image_of {image_of.shape} must be [n,4], [n,>=2] and [n]')
    hw = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    known = (image_of >= 0) & (image_of < len(hw))
    bad = ~known
    bad[known] = (hw[image_of[known]] > ARROW_SIDE).any(axis=1) | (hw[image_of[known]] <= 0).any(axis=1)
    flags = np.where(bad, 2, flags).astype(np.int32)
    if strict and flags.any():
        k = int(np.flatnonzero(flags)[0])
        raise ValueError(f'arrow {k} cannot be drawn: box {np.asarray(boxes).reshape(-1, 4)[k].tolist()}, gaze {np.asarray(gaze).reshape(len(flags), -1)[k, :2].tolist()}, '
                         f'image_of {int(image_of[k])} of {len(hw)} -- not finite, outside the image table, or an end point beyond +-{ARROW_COORD} '
                         f'/ a thickness beyond 255')
    seg[flags != 0], t[flags != 0] = 0, 0
    return seg, t, flags


def draw_arrows_host(frames, boxes, gaze, image_of=None, color=None, pixel_format='bgr', matrix='bt601', strict=False, **params):
    """The demo's arrows (MCGaze_demo/demo.ipynb, cell 5) drawn with numpy: what DevicePipeline.draw_arrows writes on the device, bit for bit
    (include/mcgaze_hip.h, "annotated frames out": the plan, the capsule coverage in 64-bit integers, the highest row winning an overlap, the
    NV12 chroma rule).  For checks and for users without a GPU.

    frames: one HxWx3 uint8 frame or a list of them; pixel_format='nv12': one surface -- a (y, uv) tuple or a [3H/2, W] array -- or a list of
    those.  boxes [n,4], gaze [n,>=2], image_of [n] (None: every row draws into frame 0), color: one (B, G, R) triple (None: the demo's
    (230, 253, 11)) or one per row; params: length, min_thickness, thickness_ratio, tip_length.
    -> (annotated COPIES in the form given -- NV12 frames as (y [H,W], uv [H/2,W]) pairs --, flags int32 [n]).  A row flagged 2 changes no
    byte; strict=True raises ValueError for it instead (what draw_arrows does for host tables)."""
    if pixel_format not in ('bgr', 'nv12'):
        raise ValueError(f"pixel_format must be 'bgr' or 'nv12', got {pixel_format!r}")
    nv12 = pixel_format == 'nv12'
    _yuv_coef(matrix)
    single = not isinstance(frames, list)
    frames = [frames] if single else frames
    if nv12:
        out = [tuple(np.array(p) for p in _nv12_planes(k, f)[:2]) for k, f in enumerate(frames)]
        sizes = [y.shape for y, _ in out]
    else:
        out = [np.array(f) for f in frames]
        for k, a in enumerate(out):
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.size == 0:
                raise TypeError(f'frame {k}: frames must be HxWx3 uint8 arrays, got {a.dtype} {a.shape}')
        sizes = [a.shape[:2] for a in out]
    n = len(np.asarray(_host_array(boxes)).reshape(-1, 4))
    image_of = np.zeros(n, dtype=np.int32) if image_of is None else _host_array(image_of)
    seg, t, flags = _arrow_rows(_host_array(boxes), _host_array(gaze), image_of, sizes, strict, **params)
    one, per_row = _arrow_colors(color, n, nv12, matrix)
    for k in np.flatnonzero(flags == 0):                         # ascending: a later row overwrites an earlier one
        h, w = sizes[int(image_of[k])]
        r = (int(t[k]) + 1) // 2
        x0, y0 = max(int(seg[k, :, :, 0].min()) - r, 0), max(int(seg[k, :, :, 1].min()) - r, 0)
        x1, y1 = min(int(seg[k, :, :, 0].max()) + r + 1, w), min(int(seg[k, :, :, 1].max()) + r + 1, h)
        if x1 <= x0 or y1 <= y0:
            continue
        mask = np.zeros((h, w), dtype=bool)
        mask[y0:y1, x0:x1] = np.logical_or.reduce([segment_coverage(y1 - y0, x1 - x0, s[0], s[1], t[k], y0, x0) for s in seg[k]])
        c = one if per_row is None else per_row[k]
        if nv12:
            y, uv = out[int(image_of[k])]
            y[mask] = c[0]
            uv.reshape(h // 2, w // 2, 2)[mask.reshape(h // 2, 2, w // 2, 2).any(axis=(1, 3))] = c[1:]
        else:
            out[int(image_of[k])][mask] = c
    return (out[0] if single else out), flags


# ---------------------------------------------------------------- head boxes from a detector's raw output (include/mcgaze_hip.h; csrc/detect.hip)
DETECT_MAX_DET = 300                                             # the reference's max_det, and the bound of the entry


def _detect_params(conf_thres=0.25, iou_thres=0.45, only_class=1, agnostic=False, max_nms=30000, max_det=300):
    """The options of detect_heads_host / DevicePipeline.detect_heads, checked -> (conf_thres, iou_thres, only_class, agnostic, max_nms, max_det)."""
    conf_thres, iou_thres = float(conf_thres), float(iou_thres)
    if not (np.isfinite(conf_thres) and np.isfinite(iou_thres)):
        raise ValueError(f'detect_heads: conf_thres and iou_thres must be finite, got {conf_thres}, {iou_thres}')
    only_class = -1 if only_class is None else int(only_class)
    if only_class < -1:
        raise ValueError(f'detect_heads: only_class is a class index, or -1 / None for every class, got {only_class}')
    if int(max_det) != max_det or not 1 <= max_det <= DETECT_MAX_DET:
        raise ValueError(f'detect_heads: max_det in 1 .. {DETECT_MAX_DET}, got {max_det}')
    if int(max_nms) != max_nms or max_nms < 1:
        raise ValueError(f'detect_heads: max_nms must be at least 1, got {max_nms}')
    return conf_thres, iou_thres, only_class, bool(agnostic), int(max_nms), int(max_det)


def _detect_shapes(shape, in_shape, frame_hw):
    """-> (B, N, nc, in_h, in_w, frame_hw [B,2] int32 or None for a device tensor, which is checked for its shape only)."""
    if len(shape) != 3 or shape[2] < 6 or shape[1] < 1:
        raise ValueError(f'detect_heads: pred must be [B, N, 5 + nc] with N >= 1 and nc >= 1, got {tuple(shape)}')
    B, N, nc = int(shape[0]), int(shape[1]), int(shape[2]) - 5
    in_h, in_w = (int(v) for v in in_shape)
    if in_h < 1 or in_w < 1:
        raise ValueError(f'detect_heads: in_shape is the detector\'s (h, w) input, got {tuple(in_shape)}')
    if isinstance(frame_hw, torch.Tensor) and frame_hw.is_cuda:
        if tuple(frame_hw.shape) != (B, 2) or frame_hw.dtype not in (torch.int32, torch.int64):
            raise ValueError(f'detect_heads: a device frame_hw is an integer [{B}, 2] tensor, got {frame_hw.dtype} {tuple(frame_hw.shape)}')
        return B, N, nc, in_h, in_w, None
    hw = _host_array(frame_hw)
    if hw.dtype.kind not in 'iu':
        raise TypeError(f'detect_heads: frame_hw must hold integers, got {hw.dtype}')
    if hw.shape == (2,):
        hw = np.broadcast_to(hw, (B, 2))
    if hw.shape != (B, 2):
        raise ValueError(f'detect_heads: frame_hw is one (h, w) or [{B}, 2], got {hw.shape}')
    return B, N, nc, in_h, in_w, np.ascontiguousarray(hw, dtype=np.int32)


def detect_heads_host(pred, in_shape, frame_hw, conf_thres=0.25, iou_thres=0.45, only_class=1, agnostic=False, max_nms=30000, max_det=300):
    """``mcg_detect_heads`` in numpy, bit for bit (the arithmetic: include/mcgaze_hip.h, "head boxes from raw detector output"): the demo's
    head detector's post-processing -- non_max_suppression on a float32 prediction with classes=[only_class] and multi_label=False, then
    scale_coords(...).round() (MCGaze_demo/yolo_head/utils/general.py:291-312, 393-481) -- for checks and for users without a GPU.

    pred [B, N, 5 + nc] (x, y, w, h, objectness, classes; f32, or fp16 which is widened exactly); in_shape: the (h, w) of the detector's
    letterboxed input; frame_hw: one (h, w) or [B, 2], the frames the boxes are scaled back into.  only_class: the head class of the
    demo's detector is 1; -1 or None keeps every class.
    -> (boxes [B, max_det, 4] f32, scores [B, max_det] f32, classes [B, max_det] int32, image_of [B, max_det] int32, counts [B] int32,
    flags [B] int32): row k < counts[b] is a detection of image b (image_of = b), best first; the rows behind are zero with image_of = -1.
    flags: 1 where more than max_nms candidates stood (the best max_nms took part), 2 for a frame without pixels (count 0)."""
    conf_thres, iou_thres, only_class, agnostic, max_nms, max_det = _detect_params(conf_thres, iou_thres, only_class, agnostic, max_nms, max_det)
    pred = _host_array(pred)
    B, N, nc, in_h, in_w, hw = _detect_shapes(pred.shape, in_shape, _host_array(frame_hw))
    if pred.dtype not in (np.float32, np.float16):
        raise TypeError(f'detect_heads: pred must be float32 or float16, got {pred.dtype}')
    pred = pred.astype(np.float32)
    f32 = np.float32
    with np.errstate(all='ignore'):
        thr, it = f32(conf_thres), f32(iou_thres)
    boxes, scores = np.zeros((B, max_det, 4), f32), np.zeros((B, max_det), f32)
    classes, image_of = np.zeros((B, max_det), np.int32), np.full((B, max_det), -1, np.int32)
    counts, flags = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        h0, w0 = int(hw[b, 0]), int(hw[b, 1])
        if h0 <= 0 or w0 <= 0:
            flags[b] = 2
            continue
        p = pred[b]
        with np.errstate(all='ignore'):
            sc = p[:, 5:] * p[:, 4:5]
            conf = sc.max(axis=1)                                # a NaN score makes conf NaN: the row is dropped below
            cls = sc.argmax(axis=1)                              # the lowest class that reaches the maximum
            half_w, half_h = p[:, 2] / f32(2), p[:, 3] / f32(2)
            box = np.stack([p[:, 0] - half_w, p[:, 1] - half_h, p[:, 0] + half_w, p[:, 1] + half_h], axis=1)
            keep = (p[:, 4] > thr) & (conf > thr) & np.isfinite(box).all(axis=1) & np.isfinite(conf)
            if only_class >= 0:
                keep &= cls == only_class
            idx = np.flatnonzero(keep)
            idx = idx[np.argsort(-(conf[idx] + f32(0)), kind='stable')]          # conf descending, ties by the lower anchor
            if len(idx) > max_nms:
                flags[b] = 1
                idx = idx[:max_nms]
            off = box[idx] + (f32(0) if agnostic else cls[idx].astype(f32) * f32(4096))[..., None]
            x1, y1, x2, y2 = off.T
            area = (x2 - x1) * (y2 - y1)
            gone, kept = np.zeros(len(idx), bool), []
            for i in range(len(idx)):
                if gone[i]:
                    continue
                kept.append(i)
                if len(kept) == max_det:
                    break
                r = slice(i + 1, None)
                w = np.maximum(f32(0), np.minimum(x2[i], x2[r]) - np.maximum(x1[i], x1[r]))
                h = np.maximum(f32(0), np.minimum(y2[i], y2[r]) - np.maximum(y1[i], y1[r]))
                inter = w * h
                gone[r] |= inter / (area[i] + area[r] - inter) > it                # NaN suppresses nothing
            rows = idx[kept]
            gain = min(in_h / h0, in_w / w0)
            pad_x, pad_y = (in_w - w0 * gain) / 2, (in_h - h0 * gain) / 2
            g, pad, hi = f32(gain), np.array([pad_x, pad_y, pad_x, pad_y], f32), np.array([w0, h0, w0, h0], f32)
            v = (box[rows] - pad) / g
            v = np.where(v < 0, f32(0), v)
            v = np.where(v > hi, hi, v)
            n = len(rows)
            boxes[b, :n], scores[b, :n], classes[b, :n], image_of[b, :n], counts[b] = np.rint(v), conf[rows], cls[rows], b, n
    return boxes, scores, classes, image_of, counts, flags


class _NoDraw:
    """The generator behind head_crop_geometry's planning pass: RandomFlip(0.0)'s uniform decides nothing and is not drawn from the caller's."""

    @staticmethod
    def random_sample():
        return 0.0


_NO_DRAW = _NoDraw()


def head_crop_windows(boxes, h, w, expand=0.8):
    """The demo's head windows (MCGaze_demo/demo.ipynb, cell 4) for n boxes at once, in the doubles python computes them in:

        head_center = [int(y1 + y2) // 2, int(x1 + x2) // 2];   l = int(max(y2 - y1, x2 - x1) * 0.8)
        head_crop = img[max(0, cy - l):min(cy + l, rows), max(0, cx - l):min(cx + l, cols)]

    boxes [n,4] x1 y1 x2 y2 (finite), h / w: frame size per box (scalars or [n]).  -> (windows int64 [n,4] = y0, x0, h, w; empty bool [n]):
    a window the slice would leave empty (a box of no extent, or wholly outside the frame) is reported as ONE pixel moved inside the frame
    and marked in ``empty`` -- what head_crop_plan_kernel (csrc/preprocess.hip) writes with flag 1; this is that kernel, line for line."""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    if not np.isfinite(b).all():
        raise ValueError('head boxes must be finite')
    l = np.trunc(np.maximum(b[:, 3] - b[:, 1], b[:, 2] - b[:, 0]) * float(expand))

    def span(a, c, size):
        size = np.broadcast_to(np.asarray(size, dtype=np.float64), a.shape)
        ctr = np.floor(np.trunc(a + c) / 2.0)        # int(a + c) // 2: truncate, then floor-divide (they differ below zero)
        lo, hi = np.maximum(0.0, ctr - l), np.minimum(ctr + l, size)
        return np.minimum(lo, size - 1), hi, ~(hi > lo)

    y0, y1, ey = span(b[:, 1], b[:, 3], h)
    x0, x1, ex = span(b[:, 0], b[:, 2], w)
    empty = ey | ex
    win = np.stack([y0, x0, np.where(empty, 1.0, y1 - y0), np.where(empty, 1.0, x1 - x0)], axis=1).astype(np.int64)
    return win, empty


def head_crop_window(box, h, w, expand=0.8):
    """(y0, x0, crop_h, crop_w) of ONE head box [x1, y1, x2, y2] in an h x w frame: the window ``DevicePipeline.head_crops`` cuts (and
    returns as ``crop``).  ValueError where the demo's slice is empty -- its cv2.resize would raise there."""
    win, empty = head_crop_windows([box], h, w, expand)
    if empty[0]:
        raise ValueError(f'head box {[float(v) for v in box]} leaves an empty window in a {h} x {w} frame')
    return tuple(int(v) for v in win[0])


def _layout(sizes, align=256):
    """Byte ranges of the given sizes laid out one behind the other, each starting on a multiple of ``align`` -> (offsets, total)."""
    offs = np.cumsum([0] + [(int(size) + align - 1) // align * align for size in sizes]).tolist()
    return offs[:-1], offs[-1]


def _device(device, entry=None):
    """torch.device(device); a bare 'cuda' is the current device BY INDEX -- staging buffers and device frames are compared with it.  With
    ``entry``, the library call about to be made, anything but a GPU is refused."""
    dev = torch.device(device)
    if entry is not None and dev.type != 'cuda':
        raise L.McgError(f'DevicePipeline runs its pixel work on the GPU ({entry}); there is no CPU path')
    return torch.device('cuda', torch.cuda.current_device()) if dev.type == 'cuda' and dev.index is None else dev


def _caller_stream(stream, dev):
    return torch.cuda.current_stream(dev) if stream is None else torch.cuda.ExternalStream(stream, device=dev)


def _kernel_norm(norm, rgb, nv12=False):
    """-> (mean, stdinv, swap) as the pixel kernels take them.  swap: the wanted order differs from the source's; converted NV12 taps are BGR."""
    mean = (C.c_float * 3)(*[float(v) for v in norm['mean']])
    stdinv = (C.c_float * 3)(*[float(np.float32(1.0 / np.float64(v))) for v in norm['std']])
    return mean, stdinv, int(bool(norm['to_rgb']) != (bool(rgb) and not nv12))


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
    """The upload stages of a DevicePipeline, used in turn, and the copy stream of each device.  What the bytes are is the caller's business:
    ``st = take(nbytes, dev, main)``, fill ``st.host`` (device addresses: ``st.base`` + offset), ``st.send(nbytes)``, launch, ``st.read_by(main)``."""

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


def _image_table(images, dev, planes):
    """-> (table, parts).  table: one _IMAGE record per frame (_NV12_IMAGE with ``planes``, the frames as _nv12_planes returns them); parts: (frame,
    field of its record, bytes) of every HOST frame -- it gets its address once it is staged.  head_crops reads the frames it names, draw_arrows
    writes them."""
    table, parts = np.zeros(len(images), dtype=_IMAGE if planes is None else _NV12_IMAGE), []
    for k, im in enumerate(images):
        if planes is not None:
            y, uv, there = planes[k]
            h, w = y.shape
            if not there:
                parts += [(k, 'y', y.reshape(-1)), (k, 'uv', uv.reshape(-1))]
            table[k] = (y.data_ptr(), uv.data_ptr(), h, w, y.stride(0), uv.stride(0) if h > 2 else w) if there else (0, 0, h, w, w, w)
        elif isinstance(im, torch.Tensor):
            if not (im.is_cuda and im.device == dev and im.dtype == torch.uint8 and im.ndim == 3 and im.shape[2] == 3 and im.numel() > 0
                    and im.stride(2) == 1 and im.stride(1) == 3 and (im.shape[0] == 1 or im.stride(0) >= 3 * im.shape[1])):
                raise TypeError(f'frame {k}: device frames must be HxWx3 uint8 tensors on {dev} with packed pixels (stride (pitch, 3, 1)), '
                                f'got {im.dtype} {tuple(im.shape)} strides {tuple(im.stride())} on {im.device}')
            table[k] = (im.data_ptr(), im.shape[0], im.shape[1], im.stride(0) if im.shape[0] > 1 else 3 * im.shape[1])
        else:
            a = np.ascontiguousarray(im)
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.size == 0:
                raise TypeError(f'frame {k}: frames must be HxWx3 uint8 arrays, got {a.dtype} {a.shape}')
            parts.append((k, 'src', a.reshape(-1)))
            table[k] = (0, a.shape[0], a.shape[1], 3 * a.shape[1])
    return table, parts


def _head_crop_tables(images, dev, planes, boxes, image_of, expand):
    """The host side of head_crops -> (table, parts, boxes, image_of, on_device, n): _image_table's frame table, and the box and index tables.
    Host tables come back in the types the device reads (f32, int32) and are CHECKED here; device tables (on_device) are not read back."""
    table, parts = _image_table(images, dev, planes)
    on_device = [isinstance(t, torch.Tensor) and t.is_cuda for t in (boxes, image_of)]
    if not on_device[0]:
        boxes = np.ascontiguousarray(_host_array(boxes), dtype=np.float32).reshape(-1, 4)     # f32 is what the device reads: the checks see the same boxes
    if not on_device[1]:
        image_of = np.ascontiguousarray(_host_array(image_of)).reshape(-1)
        if image_of.dtype.kind not in 'iu':
            raise TypeError(f'image_of must hold integers, got {image_of.dtype}')
        if len(image_of) and (image_of.min() < 0 or image_of.max() >= len(images)):
            raise ValueError(f'image_of must lie in [0, {len(images)}), got [{image_of.min()}, {image_of.max()}]')
        image_of = image_of.astype(np.int32)
    n = int(boxes.shape[0])
    if tuple(boxes.shape) != (n, 4) or tuple(image_of.shape) != (n,):
        raise ValueError(f'head_crops: boxes {tuple(boxes.shape)} and image_of {tuple(image_of.shape)} must be [n,4] and [n]')
    if n > 65535:
        raise ValueError(f'head_crops: at most 65535 crops per call (got {n})')
    if not any(on_device) and n:
        _, empty = head_crop_windows(boxes, table['h'][image_of], table['w'][image_of], expand)
        if empty.any():
            k = int(np.flatnonzero(empty)[0])
            raise ValueError(f'head box {k} {boxes[k].tolist()} leaves an empty window in frame {int(image_of[k])} '
                             f'({int(table["h"][image_of[k]])} x {int(table["w"][image_of[k]])})')
    return table, parts, boxes, image_of, on_device, n


class DevicePipeline:
    """``Compose(cfg.data.test.pipeline)`` (mmdet/datasets/pipelines/compose.py:11-51) whose pixel work is one HIP launch."""

    STAGES = 4
    IMAGE_TABLES = 16                                             # device-resident frame tables kept by head_crops (a decoder's buffer ring recurs)

    def __init__(self, transforms):
        self.transforms = [PIPELINES.build(dict(t)) if isinstance(t, dict) else t for t in transforms]
        kinds = [type(t).__name__ for t in self.transforms]
        if not kinds or kinds[0] != 'LoadImageFromFile':
            raise ValueError('the pipeline must start with LoadImageFromFile')
        if 'Normalize' not in kinds or not any(k in kinds for k in ('DefaultFormatBundle', 'ImageToTensor')) or kinds[-1] != 'Collect':
            raise ValueError(f'unsupported test pipeline {kinds}: need ... Normalize ... DefaultFormatBundle, Collect')
        self.collect = self.transforms[-1]
        self._planners = [t.plan for t in self.transforms if type(t) not in (LoadImageFromFile, ImageToTensor, Collect)]   # the rest plan nothing
        self._ring = _StagingRing(self.STAGES)                    # run_many and head_crops upload through the same stages
        self._image_tables = collections.OrderedDict()            # head_crops, draw_arrows: (device, frame table bytes) -> that table on the device
        self._frame_hw_tables = collections.OrderedDict()         # detect_heads: (device, host frame_hw bytes) -> that table on the device
        self._detect_workspaces = collections.OrderedDict()       # detect_heads: (device, B, N) -> scratch of mcg_detect_heads

    def _cached_image_table(self, table, dev, nv12):
        """The frame table ``table`` on the device: uploaded the first time these frames are seen, then found again (least recently used of
        IMAGE_TABLES goes) -- what lets head_crops and draw_arrows on device frames and tables touch the host nowhere."""
        key = (dev.index, table.tobytes()) + (('nv12',) if nv12 else ())
        tdev = self._image_tables.get(key)
        if tdev is None:
            tdev = self._image_tables[key] = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(dev)
            while len(self._image_tables) > self.IMAGE_TABLES:
                self._image_tables.popitem(last=False)
        else:
            self._image_tables.move_to_end(key)
        return tdev

    def _kept(self, cache, key, make):
        """cache[key], made the first time it is asked for; the least recently used of IMAGE_TABLES entries goes."""
        t = cache.get(key)
        if t is None:
            t = cache[key] = make()
            while len(cache) > self.IMAGE_TABLES:
                cache.popitem(last=False)
        else:
            cache.move_to_end(key)
        return t

    def plan(self, shape, rng=np.random, filename=None, ori_filename=None):
        p = FramePlan(shape, filename, ori_filename)
        for plan in self._planners:
            plan(p, rng)
        if p.pad_shape is None:
            p.pad_shape = p.img_shape
        if p.scale_factor is None:
            p.scale_factor = 1.0
        return p

    def __call__(self, frames, device='cuda:0', rng=np.random, img_prefix=None, stream=None, loader=None):
        """frames: list of HxWx3 uint8 BGR arrays (cv2 order) or file names.  Returns (img [N,3,Hp,Wp] f32 on `device`,
        img_metas list of N dicts) -- one clip batch, padded to the largest padded frame like mmcv's collate.
        loader: path -> HxWx3 uint8 array (default LoadImageFromFile.load; a FrameCache decodes ahead on host threads)."""
        return self.run_many([frames], device, rng, img_prefix, stream, loader)[0]

    def _load_and_plan(self, windows, rngs, img_prefix, loader, load, rgb_source):
        """-> (arrays, src, plans, bounds).  arrays: the DISTINCT decoded frames of this call (a file named by several windows -- they overlap
        by three frames -- is staged and uploaded once); src[k]: the array the k-th (window, frame) reads; plans stay per (window, frame): every
        use draws its own crop; window wi is rows bounds[wi]:bounds[wi + 1]."""
        arrays, src, plans, bounds, seen = [], [], [], [0], {}
        for frames, rng in zip(windows, rngs):
            for f in frames:
                if isinstance(f, str):
                    path = os.path.join(img_prefix, f) if img_prefix is not None else f
                    k = seen.get(path)
                    if k is None:
                        arr = load(path)
                        if not rgb_source and getattr(loader, 'rgb', False):
                            arr = np.ascontiguousarray(arr[..., ::-1])       # mixed with caller-supplied BGR arrays: one order per call
                        k = seen[path] = len(arrays)
                        arrays.append(arr)
                    arr, names = arrays[k], (path, f)
                else:
                    arr, names = np.ascontiguousarray(f), (None, None)
                    k = len(arrays)
                    arrays.append(arr)
                if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
                    raise TypeError(f'frames must be HxWx3 uint8 arrays, got {arr.dtype} {arr.shape}')
                src.append(k)
                plans.append(self.plan(arr.shape, rng, *names))
            bounds.append(len(src))
        return arrays, src, plans, bounds

    def run_many(self, windows, device='cuda:0', rng=np.random, img_prefix=None, stream=None, loader=None):
        """Several clip batches (windows) through ONE staging copy and one launch per distinct padded size: windows = list of lists
        of frames (arrays or file names) -> list of (img, img_metas), each exactly what ``__call__`` returns for that window -- frames
        are planned window by window, frame by frame, so the RNG draws fall where they do one window at a time; padding is per
        window (mmcv's collate pads a clip to ITS largest frame)."""
        lib, release = L.load(), getattr(loader, 'release', lambda: None)
        dev = _device(device, 'mcg_preprocess_frames')
        rgb_source = all(isinstance(f, str) for w in windows for f in w)      # our own decode: keep PIL's RGB order, the kernel swaps
        if loader is not None:
            load = loader
            rgb_source = rgb_source and bool(getattr(loader, 'rgb', False))
        else:
            load = (lambda path: LoadImageFromFile.load(path, rgb=True)) if rgb_source else LoadImageFromFile.load
        rngs = rng if isinstance(rng, (list, tuple)) else [rng] * len(windows)   # one generator per window (harness: one per VIDEO), or one for all
        if len(rngs) != len(windows):
            raise ValueError(f'run_many: {len(rngs)} generators for {len(windows)} windows')
        try:
            arrays, src, plans, bounds = self._load_and_plan(windows, rngs, img_prefix, loader, load, rgb_source)
            out = [None if bounds[wi + 1] > bounds[wi] else (torch.empty(0, 3, 0, 0, dtype=torch.float32, device=dev), []) for wi in range(len(windows))]
            if not src:
                return out
            groups = {}                                           # padded size -> windows
            for wi in range(len(windows)):
                a, b = bounds[wi], bounds[wi + 1]
                if b > a:
                    pad = (max(p.pad_shape[0] for p in plans[a:b]), max(p.pad_shape[1] for p in plans[a:b]))
                    groups.setdefault(pad, []).append(wi)
            rows = {pad: np.concatenate([np.arange(bounds[wi], bounds[wi + 1]) for wi in wis]) for pad, wis in groups.items()}
            # the frame descriptors travel in the same pinned staging buffer, behind the pixels: one non-blocking copy for everything (a
            # pageable .to() per descriptor table blocked the host until the stream had drained -- the engine's previous batch)
            dsz = C.sizeof(L.FrameDesc)
            offs, total = _layout([a.size for a in arrays] + [len(idx) * dsz for idx in rows.values()])
            desc_off = dict(zip(groups, offs[len(arrays):]))
            with torch.cuda.device(dev):
                main = _caller_stream(stream, dev)
                st = self._ring.take(total, dev, main)
                for a, o in zip(arrays, offs):
                    st.host[o:o + a.size] = a.reshape(-1)
                release()                                         # ring views of a FrameCache: copied, their slots may go
                # descriptors (mcg_frame_desc), built as one structured array per padded size
                addr = st.base + np.asarray(offs[:len(arrays)], dtype=np.int64)[src]
                shp = np.asarray([a.shape[:2] for a in arrays], dtype=np.int32)[src]
                geo = np.asarray([p.crop + p.img_shape[:2] for p in plans], dtype=np.int32)          # crop y, x, h, w, out h, w
                for pad, idx in rows.items():
                    desc = np.zeros(len(idx), dtype=_DESC)
                    desc['src'], desc['src_h'], desc['src_w'], desc['src_pitch'] = addr[idx], shp[idx, 0], shp[idx, 1], shp[idx, 1] * 3
                    for j, f in enumerate(('crop_y', 'crop_x', 'crop_h', 'crop_w', 'out_h', 'out_w')):
                        desc[f] = geo[idx, j]
                    st.host[desc_off[pad]:desc_off[pad] + len(idx) * dsz] = desc.view(np.uint8)
                st.send(total)
            mean, stdinv, swap = _kernel_norm(plans[0].img_norm_cfg, rgb_source)
            for (pad_h, pad_w), wis in groups.items():
                n = len(rows[pad_h, pad_w])
                img = torch.empty(n, 3, pad_h, pad_w, dtype=torch.float32, device=dev)
                L.check(lib.mcg_preprocess_frames(C.c_void_p(main.cuda_stream), C.c_void_p(st.base + desc_off[(pad_h, pad_w)]), n, C.c_void_p(img.data_ptr()),
                                                  pad_h, pad_w, mean, stdinv, swap), 'mcg_preprocess_frames')
                for wi, part in zip(wis, img.split([bounds[wi + 1] - bounds[wi] for wi in wis])):
                    out[wi] = (part, [self.collect.meta(p) for p in plans[bounds[wi]:bounds[wi + 1]]])
            st.read_by(main)
            return out
        except BaseException:
            # a TypeError for a non-uint8 frame, a decode error, a staging failure: the ring views handed out so far are not read any more --
            # without this they stayed pinned and a caller that carried on met 'all cached frames are handed out' later
            release()
            raise

    def head_crop_geometry(self):
        """-> (scale_w, scale_h, pad_h, pad_w, img_norm_cfg) of the chain a head crop goes through, which must be the demo's
        ``cfg.data.test.pipeline[1:]``: Resize(keep_ratio=True), no flip, Normalize, Pad -- NotImplementedError for anything else."""
        kinds = [type(t).__name__ for t in self.transforms]
        if 'CenterCrop' in kinds:
            raise NotImplementedError('head_crops: the window comes from the head box; a pipeline with a CenterCrop is not the demo\'s chain')
        resize = next((t for t in self.transforms if isinstance(t, Resize)), None)
        if resize is None or not resize.keep_ratio or resize.img_scale[0] != resize.img_scale[1]:
            raise NotImplementedError('head_crops needs Resize(img_scale=(s, s), keep_ratio=True): a window clipped by the frame border may be '
                                      'upright or lying, and keep_ratio puts the long edge of img_scale on its long side')
        scale_w, scale_h = resize.img_scale
        p = self.plan((scale_h, scale_w, 3), _NO_DRAW)            # the LARGEST resized crop through the planners: its pad_shape holds every crop
        return int(scale_w), int(scale_h), int(p.pad_shape[0]), int(p.pad_shape[1]), p.img_norm_cfg

    def head_crops(self, images, boxes, image_of, expand=0.8, device='cuda:0', stream=None, rgb=False, pixel_format='bgr', matrix='bt601'):
        """Video frames and head boxes -> the model's input, one head crop per box (MCGaze_demo/demo.ipynb, cell 4, then this chain): ONE
        plan launch chooses every window on the device, the pixel kernel reads it (mcg_preprocess_head_crops).

        images: list of HxWx3 uint8 frames in cv2's BGR order (rgb=True: RGB, the kernel swaps either way).  A numpy array is staged and
        uploaded ONCE however many heads it shows; a CUDA uint8 tensor is read where it is (rows stride(0) bytes apart, pixels packed).
        boxes [n,4] f32 x1 y1 x2 y2 in pixels of their frame; image_of [n] int: the frame of each box -- numpy arrays or device tensors.
        Host tables are checked here (ValueError for an image_of out of range, a non-finite box or a window the demo's
        slice leaves empty); device tables are not read back -- such rows come back flagged instead (1: empty window, cut as one pixel
        inside the frame; 2: unusable box / index, pixel (0, 0) of frame 0), and a call on device frames and tables touches the host
        nowhere: it can be captured in a graph once a first call has uploaded the frame table (kept per distinct set of frames).

        -> (img [n,3,Hp,Wp] f32, img_hw [n,2] int32, scale_factor [n,4] f32, crop [n,4] int32 = y0, x0, h, w, flags [n] int32), all on
        the device.  (Hp, Wp) is img_scale rounded up by Pad -- for every call, where mmcv's collate pads a chunk to ITS largest crop (the
        same unless the frame border clips every crop of the chunk on one axis); img_hw is each crop's true resized size, the reference's
        img_shape, and the decoder clips by it.

        pixel_format='nv12': the frames are a video decoder's NV12 surfaces and are read as they are (mcg_preprocess_head_crops_nv12 converts
        each tap it samples; no BGR frame is ever written).  Each image is a (y [H,W], uv [H/2,W/2,2] or [H/2,W]) pair or ONE [3H/2, W] surface
        (the Y rows, then the UV rows), uint8, H and W even: numpy arrays are staged in the same single copy, CUDA tensors are read in place
        (row strides are the pitches, at least W; bytes inside a row are packed).  matrix: 'bt601' (cv2's COLOR_YUV2BGR_NV12 constants) or
        'bt709' (what HD decoders emit), both limited range -- ``YUV_COEF``.  rgb= is ignored: the output order is the config's to_rgb.  TypeError
        / ValueError for a wrong dtype, rank, device or plane shape and for odd sizes, before anything is launched.  The result equals
        head_crops on ``nv12_to_bgr`` of the same planes bit for bit; tables, flags and the no-host-touch property are as for BGR."""
        lib = L.load()
        if pixel_format not in ('bgr', 'nv12'):
            raise ValueError(f"pixel_format must be 'bgr' or 'nv12', got {pixel_format!r}")
        coef = _yuv_coef(matrix)
        nv12 = pixel_format == 'nv12'
        dev = _device(device)                                     # the surfaces are checked whatever the device: a bad one is the caller's first error
        planes = [_nv12_planes(k, im, dev) for k, im in enumerate(images)] if nv12 else None
        dev = _device(dev, 'mcg_preprocess_head_crops')
        scale_w, scale_h, pad_h, pad_w, norm = self.head_crop_geometry()
        if not len(images):
            raise ValueError('head_crops: no frames')
        table, parts, boxes, image_of, on_device, n = _head_crop_tables(images, dev, planes, boxes, image_of, expand)
        with torch.cuda.device(dev):
            main = _caller_stream(stream, dev)
            with torch.cuda.stream(main):
                boxes = boxes.to(dev, torch.float32).contiguous() if on_device[0] else boxes
                image_of = image_of.to(dev, torch.int32).contiguous() if on_device[1] else image_of
                new = lambda *shape, dtype=torch.int32: torch.empty(*shape, dtype=dtype, device=dev)
                if n == 0:
                    return new(0, 3, pad_h, pad_w, dtype=torch.float32), new(0, 2), new(0, 4, dtype=torch.float32), new(0, 4), new(0)
                # everything that comes from the host travels in ONE pinned staging buffer and one copy: pixels, frame table, host tables
                tables = [t.view(np.uint8).reshape(-1) for t, d in zip((boxes, image_of), on_device) if not d]
                st = None
                if parts or tables:
                    blobs = [a for _, _, a in parts] + [table.view(np.uint8).reshape(-1)] + tables     # (the table's bytes are a VIEW: filled below, then copied)
                    offs, total = _layout([b.size for b in blobs])
                    st = self._ring.take(total, dev, main)
                    for (k, f, _), o in zip(parts, offs):
                        table[f][k] = st.base + o                 # a host frame's address: where its bytes land in the device twin
                    for b, o in zip(blobs, offs):
                        st.host[o:o + b.size] = b
                    st.send(total)
                    at = [st.base + o for o in offs[len(parts):]]                                # frame table, then the host tables
                    images_ptr = at.pop(0)
                    boxes_ptr = boxes.data_ptr() if on_device[0] else at.pop(0)
                    image_of_ptr = image_of.data_ptr() if on_device[1] else at.pop(0)
                else:
                    # nothing comes from the host but the frame table, and that only the first time these frames are seen: no stage is taken
                    tdev = self._cached_image_table(table, dev, nv12)
                    images_ptr, boxes_ptr, image_of_ptr = tdev.data_ptr(), boxes.data_ptr(), image_of.data_ptr()
                img, scale_factor = new(n, 3, pad_h, pad_w, dtype=torch.float32), new(n, 4, dtype=torch.float32)
                desc, img_hw, flags = new(n, _NV12_DESC_WORDS if nv12 else _DESC_WORDS), new(n, 2), new(n)
                vp = C.c_void_p
                entry, more = (lib.mcg_preprocess_head_crops_nv12, (C.byref(L.YuvCoef(**coef)),)) if nv12 else (lib.mcg_preprocess_head_crops, ())
                L.check(entry(vp(main.cuda_stream), vp(images_ptr), len(images), vp(boxes_ptr), vp(image_of_ptr), n, float(expand),
                              scale_w, scale_h, vp(desc.data_ptr()), vp(img_hw.data_ptr()), vp(scale_factor.data_ptr()),
                              vp(flags.data_ptr()), vp(img.data_ptr()), pad_h, pad_w, *_kernel_norm(norm, rgb, nv12), *more), entry.__name__)
                if st is not None:
                    st.read_by(main)
        return img, img_hw, scale_factor, desc[:, _CROP_WORD:_CROP_WORD + 4], flags

    def draw_arrows(self, images, boxes, gaze, image_of, color=None, pixel_format='bgr', matrix='bt601', copy=False, device='cuda:0', stream=None,
                    **params):
        """The demo's last step (MCGaze_demo/demo.ipynb, cell 5) on the device: one arrow per head, from the head's centre along its gaze, drawn
        into the frames (mcg_draw_gaze_arrows / mcg_draw_gaze_arrows_nv12: a plan launch and a raster launch) -- ``draw_arrows_host`` bit for bit.

        images: as for head_crops -- HxWx3 uint8 frames, or with pixel_format='nv12' (y, uv) pairs / [3H/2, W] surfaces; numpy arrays or CUDA
        tensors.  A CUDA frame is drawn IN PLACE (copy=True: into a packed clone) and handed back as it was given; a numpy frame goes up through the
        staging ring into a fresh device tensor (NV12: one [3H/2, W] surface, handed back as its (y [H,W], uv [H/2,W]) views), which is drawn into.
        boxes [n,4] x1 y1 x2 y2, gaze [n,>=2] (only g0, g1 are read), image_of [n]: numpy arrays or device tensors; an f32 device gaze with packed
        rows -- the [n,3] ``fused`` of a results='device' stream -- is read where it is, its row stride taken from the tensor.
        color: one (B, G, R) triple (None: the demo's (230, 253, 11)) or one per row, [n,3], on the host; for NV12 each is converted once by
        ``bgr_to_yuv(color, matrix)``.  params: length, min_thickness, thickness_ratio, tip_length (the demo's 1.0, 5, 0.01, 0.1).
        Where arrows overlap the highest row wins.  Host tables are checked before anything is launched (ValueError: an image_of out of range, a
        box or gaze that is not finite, an end point beyond +-8191 or a thickness beyond 255; a frame larger than 8192 a side); device tables are
        not read back -- such rows come back with flag 2 and write nothing.  TypeError / ValueError for frames as in head_crops.  With device
        frames drawn in place, device tables and one colour the call touches the host nowhere once a first call has uploaded the frame table (the
        cache head_crops keeps): it can be captured in a graph.
        -> (images on the device, in order; flags [n] int32 on the device: 0 drawn -- possibly no pixel --, 2 unusable)."""
        lib = L.load()
        if pixel_format not in ('bgr', 'nv12'):
            raise ValueError(f"pixel_format must be 'bgr' or 'nv12', got {pixel_format!r}")
        _yuv_coef(matrix)
        length, min_thickness, ratio, tip_length = _arrow_params(**params)
        nv12 = pixel_format == 'nv12'
        entry = lib.mcg_draw_gaze_arrows_nv12 if nv12 else lib.mcg_draw_gaze_arrows
        dev = _device(device)
        images = list(images)
        planes = [_nv12_planes(k, im, dev) for k, im in enumerate(images)] if nv12 else None
        dev = _device(dev, entry.__name__)
        if not len(images):
            raise ValueError('draw_arrows: no frames')
        table, _ = _image_table(images, dev, planes)              # every frame is checked before the first clone or upload
        on_device = [isinstance(t, torch.Tensor) and t.is_cuda for t in (boxes, gaze, image_of)]
        if not on_device[0]:
            boxes = np.ascontiguousarray(_host_array(boxes), dtype=np.float32).reshape(-1, 4)
        n = int(boxes.shape[0])
        if not on_device[1]:
            gaze = np.ascontiguousarray(_host_array(gaze), dtype=np.float32)
            gaze = np.zeros((0, 2), np.float32) if n == 0 and gaze.size == 0 else np.ascontiguousarray(gaze[:, :2]) if gaze.ndim == 2 else gaze
        if not on_device[2]:
            image_of = np.ascontiguousarray(_host_array(image_of)).reshape(-1)
            if image_of.dtype.kind not in 'iu':
                raise TypeError(f'image_of must hold integers, got {image_of.dtype}')
            if len(image_of) and (image_of.min() < 0 or image_of.max() >= len(images)):
                raise ValueError(f'image_of must lie in [0, {len(images)}), got [{image_of.min()}, {image_of.max()}]')
            image_of = image_of.astype(np.int32)
        if tuple(boxes.shape) != (n, 4) or gaze.ndim != 2 or gaze.shape[0] != n or gaze.shape[1] < 2 or tuple(image_of.shape) != (n,):
            raise ValueError(f'draw_arrows: boxes {tuple(boxes.shape)}, gaze {tuple(gaze.shape)} and image_of {tuple(image_of.shape)} must be [n,4], [n,>=2] and [n]')
        if n > 65535:
            raise ValueError(f'draw_arrows: at most 65535 arrows per call (got {n})')
        for name, t, there in (('box', boxes, on_device[0]), ('gaze', gaze, on_device[1])):
            if not there and not np.isfinite(t).all():
                raise ValueError(f'draw_arrows: {name} {int(np.flatnonzero(~np.isfinite(t).all(axis=1))[0])} is not finite')
        one, per_row = _arrow_colors(color, n, nv12, matrix)
        with torch.cuda.device(dev):
            main = _caller_stream(stream, dev)
            with torch.cuda.stream(main):
                # where the arrows go: a device frame itself (or its clone), a fresh device tensor for every host frame
                out = []
                for k, im in enumerate(images):
                    if nv12 and not planes[k][2]:
                        h, w = planes[k][0].shape
                        s = torch.empty(h * 3 // 2, w, dtype=torch.uint8, device=dev)
                        out.append((s[:h], s[h:]))
                    elif not nv12 and not isinstance(im, torch.Tensor):
                        out.append(torch.empty(np.shape(im), dtype=torch.uint8, device=dev))
                    elif copy:
                        clone = lambda t: t.clone(memory_format=torch.contiguous_format)
                        out.append(tuple(clone(t) for t in im) if isinstance(im, (tuple, list)) else clone(im))
                    else:
                        out.append(im)
                in_place = all(o is im for o, im in zip(out, images))
                if not in_place:                                  # the table of the tensors that are drawn into
                    table, _ = _image_table(out, dev, [_nv12_planes(k, o, dev) for k, o in enumerate(out)] if nv12 else None)
                if table['h'].max() > ARROW_SIDE or table['w'].max() > ARROW_SIDE:
                    raise ValueError(f'draw_arrows: frames of at most {ARROW_SIDE} pixels a side, got {int(table["h"].max())} x {int(table["w"].max())}')
                if not any(on_device[:2]) and n:
                    _arrow_rows(boxes, gaze, image_of if not on_device[2] else np.zeros(n, np.int32),
                                [(int(r['h']), int(r['w'])) for r in table], True, length=length, min_thickness=min_thickness,
                                thickness_ratio=ratio, tip_length=tip_length)
                boxes = boxes.to(dev, torch.float32).contiguous() if on_device[0] else boxes
                image_of = image_of.to(dev, torch.int32).contiguous() if on_device[2] else image_of
                if on_device[1]:
                    if not (gaze.device == dev and gaze.dtype == torch.float32 and gaze.stride(1) == 1 and (n <= 1 or gaze.stride(0) >= 2)):
                        gaze = gaze.to(dev, torch.float32).contiguous()
                    gaze_stride = int(gaze.stride(0)) if n > 1 else int(gaze.shape[1])
                else:
                    gaze_stride = 2
                # the bytes of the host frames (frame, the device tensor they belong in, bytes), in image order
                if nv12:
                    pixels = [(o[j], a.reshape(-1)) for o, p in zip(out, planes) if not p[2] for j, a in enumerate(p[:2])]
                else:
                    pixels = [(o, np.ascontiguousarray(im).reshape(-1)) for o, im in zip(out, images) if not isinstance(im, torch.Tensor)]
                tables = [t.view(np.uint8).reshape(-1) for t, d in zip((boxes, gaze, image_of), on_device) if not d] + ([] if per_row is None else [per_row.reshape(-1)])
                st = None
                if pixels or tables or not in_place:
                    # everything that comes from the host travels in ONE pinned staging buffer and one copy: pixels, frame table, host tables
                    blobs = [a for _, a in pixels] + [table.view(np.uint8).reshape(-1)] + tables
                    offs, total = _layout([b.size for b in blobs])
                    st = self._ring.take(total, dev, main)
                    for b, o in zip(blobs, offs):
                        st.host[o:o + b.size] = b
                    st.send(total)
                    for (dst, a), o in zip(pixels, offs):          # out of the stage (the next calls reuse it) into the tensor handed back
                        dst.copy_(st.dev[o:o + a.size].view(dst.shape))
                    at = [st.base + o for o in offs[len(pixels):]]
                    images_ptr = at.pop(0)
                    boxes_ptr = boxes.data_ptr() if on_device[0] else at.pop(0)
                    gaze_ptr = gaze.data_ptr() if on_device[1] else at.pop(0)
                    image_of_ptr = image_of.data_ptr() if on_device[2] else at.pop(0)
                    colors_ptr = None if per_row is None else at.pop(0)
                else:
                    # device frames drawn in place, device tables, one colour: only the frame table, and only the first time the frames are seen
                    tdev = self._cached_image_table(table, dev, nv12)
                    images_ptr, boxes_ptr, gaze_ptr, image_of_ptr, colors_ptr = tdev.data_ptr(), boxes.data_ptr(), gaze.data_ptr(), image_of.data_ptr(), None
                flags = torch.empty(n, dtype=torch.int32, device=dev)
                if n:
                    plan = torch.empty(n, _ARROW_WORDS, dtype=torch.int32, device=dev)
                    vp = C.c_void_p
                    L.check(entry(vp(main.cuda_stream), vp(images_ptr), len(out), int(table['h'].max()), int(table['w'].max()), vp(boxes_ptr), vp(gaze_ptr),
                                  gaze_stride, vp(image_of_ptr), n, length, min_thickness, ratio, tip_length,
                                  None if one is None else (C.c_ubyte * 3)(*[int(v) for v in one]), vp(colors_ptr), vp(plan.data_ptr()),
                                  vp(flags.data_ptr())), entry.__name__)
                if st is not None:
                    st.read_by(main)
        return out, flags

    def detect_heads(self, pred, in_shape, frame_hw, conf_thres=0.25, iou_thres=0.45, only_class=1, agnostic=False, max_nms=30000, max_det=300,
                     device='cuda:0', stream=None):
        """Head boxes from the raw output of the demo's head detector, on the device (mcg_detect_heads: one launch, one workgroup per image) --
        ``detect_heads_host`` bit for bit: the confidence filter, class-aware greedy NMS and the scale-back into the frame of
        non_max_suppression + scale_coords(...).round() (MCGaze_demo/yolo_head/detect.py:74,95).

        pred [B, N, 5 + nc]: a CUDA tensor is read where it is, its image and row strides taken from the tensor (fp16 is widened with
        ``.float()``, which is exact; anything but unit-stride rows is made contiguous first); a numpy array goes up through the staging ring.
        in_shape: the (h, w) of the detector's letterboxed input.  frame_hw: one (h, w), an [B, 2] array, or an integer [B, 2] device tensor
        (h0, w0 per image), which is not read back.  The other arguments are detect_heads_host's; they and the shapes are checked before
        anything is launched (TypeError / ValueError).
        -> (boxes [B, max_det, 4] f32, scores [B, max_det] f32, classes, image_of [B, max_det] int32, counts [B] int32, flags [B] int32) on the
        device.  Rows behind counts[b] are zero with image_of = -1, which head_crops and draw_arrows flag as unusable rows: ``boxes.view(-1, 4)``
        and ``image_of.view(-1)`` feed them with no read-back.  The workspace is kept per (B, N) and the table of a host frame_hw per
        content, so a call on a device prediction touches the host nowhere after the first and can be captured in a graph; calls that share a
        (B, N) share the workspace and belong on one stream."""
        lib = L.load()
        params = _detect_params(conf_thres, iou_thres, only_class, agnostic, max_nms, max_det)
        conf_thres, iou_thres, only_class, agnostic, max_nms, max_det = params
        on_device = isinstance(pred, torch.Tensor) and pred.is_cuda
        if not on_device:
            pred = _host_array(pred)
        if pred.dtype not in ((torch.float32, torch.float16) if on_device else (np.float32, np.float16)):
            raise TypeError(f'detect_heads: pred must be float32 or float16, got {pred.dtype}')
        B, N, nc, in_h, in_w, hw = _detect_shapes(tuple(pred.shape), in_shape, frame_hw)
        dev = _device(pred.device if on_device else device, 'mcg_detect_heads')
        with torch.cuda.device(dev):
            main = _caller_stream(stream, dev)
            with torch.cuda.stream(main):
                new = lambda *shape, dtype=torch.int32: torch.empty(*shape, dtype=dtype, device=dev)
                out = (new(B, max_det, 4, dtype=torch.float32), new(B, max_det, dtype=torch.float32), new(B, max_det), new(B, max_det), new(B), new(B))
                if B == 0:
                    return out
                st = None
                if on_device:
                    pred = pred.float()
                    if pred.stride(2) != 1 or pred.stride(1) < 5 + nc or pred.stride(0) < 0:
                        pred = pred.contiguous()
                    pred_ptr, image_stride, row_stride = pred.data_ptr(), int(pred.stride(0)), int(pred.stride(1))
                else:
                    flat = np.ascontiguousarray(pred, dtype=np.float32).reshape(-1).view(np.uint8)
                    st = self._ring.take(flat.size, dev, main)
                    st.host[:flat.size] = flat
                    st.send(flat.size)
                    pred_ptr, image_stride, row_stride = st.base, N * (5 + nc), 5 + nc
                if hw is None:
                    frame_hw = frame_hw.to(torch.int32).contiguous()
                else:
                    frame_hw = self._kept(self._frame_hw_tables, (dev.index, hw.tobytes()), lambda: torch.from_numpy(hw.copy()).to(dev))
                ws = self._kept(self._detect_workspaces, (dev.index, B, N),
                                lambda: torch.empty(int(lib.mcg_detect_heads_workspace_bytes(B, N)), dtype=torch.uint8, device=dev))
                vp = C.c_void_p
                L.check(lib.mcg_detect_heads(vp(main.cuda_stream), vp(pred_ptr), B, N, nc, image_stride, row_stride, in_h, in_w, vp(frame_hw.data_ptr()),
                                             conf_thres, iou_thres, only_class, int(agnostic), min(max_nms, N), max_det, *(vp(t.data_ptr()) for t in out),
                                             vp(ws.data_ptr()), ws.numel()), 'mcg_detect_heads')
                if st is not None:
                    st.read_by(main)
        return out


def _host_array(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def build_pipeline(transforms):
    return DevicePipeline(transforms)

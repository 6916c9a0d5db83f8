"""Decoded frames: the PIL decode behind ``LoadImageFromFile.load``, and ``FrameCache``, which shares one decode among the windows that use a
frame and can decode ahead -- on host threads, or in helper processes (``_DecodeProcs``, _decode_worker.py) that fill a shared-memory ring."""
import collections
import concurrent.futures
import os
import struct
import threading
import time

import numpy as np


def decode_image(filename, rgb=False):
    """-> HxWx3 uint8, BGR like cv2.imread's (rgb=True: the decoder's RGB order as it is -- the pixel kernel swaps channels
    either way, and the per-frame flip copy is saved)."""
    from PIL import Image
    with Image.open(filename) as im:
        arr = np.asarray(im.convert('RGB'))
    return arr if rgb else np.ascontiguousarray(arr[..., ::-1])


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
        self.loader = loader or (lambda path: decode_image(path, rgb=True))
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

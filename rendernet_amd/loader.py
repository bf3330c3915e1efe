"""Prefetching uint8 training loader: the batches of `tools.data_util.data_loader` + the script's slicing, delivered as
bytes through pinned memory while the previous step runs.

Two layers.

`iter_host_batches` (host only, no GPU): one reader thread streams the image tar, `workers` threads decode PNG/JPG
pixels (PIL releases the GIL), the generator assembles -- per optimiser step and for ONE rank's shard -- exactly the
samples today's script would have trained on at that step, as decoded bytes: no float conversion, no mean over the
channels, no division; those happen on the device (`ops.target_u8_crop`, rn_target_u8_crop_fwd).  Binvox models are
decoded once and kept as uint8 in an LRU cache.

`PrefetchLoader` (device): `depth` slots of pinned host memory and of device memory, filled by a producer thread with
non-blocking copies on one side stream and handed to the consumer with events -- no host synchronise on the consumer
side.

The sequence is defined by the composition it replaces (RenderNet_Shader.py:193-240 on tools/data_util.py:64-157): chunks
of batch_size * batches_chunk samples in tar order; a final short chunk of n samples gives n // batch_size batches when
n is a multiple of batch_size, and otherwise ONE batch -- its first batch_size samples when n > batch_size, its samples
repeated element-wise (s0 s0 s1 s1 ...) up to batch_size when n < batch_size.  Because a complete batch after the first
may still be dropped by that rule, the batches of a chunk are yielded when the chunk closes; decoding of the next chunk
overlaps their consumption (up to two chunks of this rank's decoded bytes are alive at a time, a fraction of the float32
chunk the synchronous loader holds).
"""
import collections
import io
import queue
import tarfile
import threading
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .tools import binvox_rw
from .tools import data_util

MAX_WORKERS = 16                     # hard cap on decode threads; the count is an argument, never the machine's CPU count
_IMAGE_KINDS = ('jpg', 'jpeg', 'png')
# what tools.utils.NpyTarReader treats as "unreadable image -> skip"
_UNREADABLE = (OSError, RuntimeError, TypeError, ValueError)
_END = object()
_POLL = 0.05                         # seconds between looks at the stop flag while blocked on a queue


class _Failure(object):
    def __init__(self, exc):
        self.exc = exc


def _open_header(raw):
    """Image.open is lazy: it parses the header only."""
    from PIL import Image
    return Image.open(io.BytesIO(raw))


def _decode_pixels(raw):
    """The pixel decode of tools.utils.NpyTarReader without its float32 cast."""
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(raw)))


def _read_binvox(path):
    with open(path, 'rb') as f:
        return np.reshape(binvox_rw.read_as_3d_array(f).data, (64, 64, 64, 1)).astype(np.uint8)


class _ModelCache(object):
    """LRU of decoded models (262 KB each) keyed by file path.  The read happens under the lock so that two workers
    asking for the same model read it once."""

    def __init__(self, capacity):
        self.capacity = max(1, int(capacity))
        self.lock = threading.Lock()
        self.models = collections.OrderedDict()

    def get(self, path):
        with self.lock:
            vox = self.models.get(path)
            if vox is None:
                vox = self.models[path] = _read_binvox(path)
                if len(self.models) > self.capacity:
                    self.models.popitem(last=False)
            else:
                self.models.move_to_end(path)
            return vox


class _Sample(object):
    """One counted member of the tar: its name and either a decode in flight (`fut`), or the member's bytes kept in case
    the tail rule hands the sample to this rank after all (`raw`), or neither (another rank's sample)."""
    __slots__ = ("name", "fut", "raw")

    def __init__(self, name, fut=None, raw=None):
        self.name, self.fut, self.raw = name, fut, raw


def _decode_sample(raw, name, model_path, flatten, img_res, cache, strict):
    """(pixels uint8 [res,res,Cs], voxels uint8 [64,64,64,1], pose float32 [3]) of one member, or None for an image that
    does not decode (strict=False: the synchronous loader's skip).  strict=True raises instead, naming the member."""
    try:
        px = _decode_pixels(raw)
    except _UNREADABLE as e:
        if not strict:
            return None
        raise RuntimeError("image member %r: the header opens but the pixels do not decode (%s).  With more than one rank "
                           "the other ranks have already counted this sample; remove the member from the tar" % (name, e))
    if px.dtype == np.bool_:
        px = px.astype(np.uint8)
    if px.dtype != np.uint8:
        raise ValueError("image member %r decodes to %s; the uint8 loader takes 8-bit images only" % (name, px.dtype))
    if px.ndim == 2:
        px = px[:, :, None]
    if px.ndim != 3 or px.shape[:2] != (img_res, img_res) or px.shape[2] not in (1, 3, 4) or (not flatten and px.shape[2] < 3):
        raise ValueError("image member %r has shape %s; expected %dx%d with %s channels"
                         % (name, px.shape, img_res, img_res, "1, 3 or 4" if flatten else "3 or 4"))
    pose = np.asarray(data_util.extract_param_from_names(name)[0], np.float32)
    vox = cache.get(data_util.model_file_for(name, model_path))
    return np.ascontiguousarray(px), vox, pose


def _put(q, stop, item):
    while not stop.is_set():
        try:
            q.put(item, timeout=_POLL)
            return True
        except queue.Full:
            pass
    return False


def _get(q, stop):
    while not stop.is_set():
        try:
            return q.get(timeout=_POLL)
        except queue.Empty:
            pass
    return None


def _read_members(img_path, q, stop, submit, bs, chunk, lo, hi, world):
    """Reader thread: stream the tar (it is a sequential `r|` stream), hand every image member on as a _Sample in tar
    order.  world == 1: every member is decoded (whether it counts is known only after its pixels decoded).  world > 1:
    a member counts when its HEADER opens -- every rank can tell without decoding -- and only this rank's positions of
    the batch are decoded; the bytes of the other positions of a chunk's first batch are kept until the chunk closes,
    because the tail rule can re-deal exactly those."""
    try:
        tfile = tarfile.open(img_path, 'r|')
        try:
            counted = 0
            for entry in tfile:
                if stop.is_set():
                    return
                if not entry.isfile():
                    continue
                ext = entry.name.split('.')
                packed = ext[-1].lower() == 'z'
                if packed:
                    ext.pop()
                if ext[-1].lower() not in _IMAGE_KINDS:
                    continue
                raw = tfile.extractfile(entry).read()
                if packed:
                    raw = zlib.decompress(raw)
                name = entry.name[:-(len(ext[-1]) + 1)].rsplit('/', 1)[-1]       # as tools.utils.NpyTarReader names it
                if world == 1:
                    sample = _Sample(name, fut=submit(raw, name, False))
                else:
                    try:
                        _open_header(raw)
                    except _UNREADABLE:
                        continue
                    i = counted % chunk
                    counted += 1
                    if lo <= i % bs < hi:
                        sample = _Sample(name, fut=submit(raw, name, True))
                    else:
                        sample = _Sample(name, raw=raw if i < bs else None)
                if not _put(q, stop, sample):
                    return
        finally:
            tfile.close()
        _put(q, stop, _END)
    except BaseException as e:                                   # surfaces from next() in the consumer
        _put(q, stop, _Failure(e))


def _batch(results, names):
    chans = [r[0].shape[2] for r in results]
    for c, n in zip(chans, names):
        if c != chans[0]:
            raise ValueError("image member %r has %d channels, the first of its batch (%r) has %d: one batch is one "
                             "channel count" % (n, c, names[0], chans[0]))
    return (np.stack([r[0] for r in results]), np.stack([r[1] for r in results]), np.stack([r[2] for r in results]),
            list(names))


def _host_batches(cfg, img_path, model_path, flatten, img_res, rank, world, workers, model_cache):
    from .parallel import shard_range
    bs = int(cfg['batch_size'])
    chunk = bs * int(cfg['batches_chunk'])
    lo, hi = shard_range(bs, rank, world)
    cache = _ModelCache(model_cache)
    stop = threading.Event()
    q = queue.Queue(maxsize=chunk)
    pool = ThreadPoolExecutor(max_workers=workers, thread_name_prefix="rn-decode")

    def submit(raw, name, strict):
        return pool.submit(_decode_sample, raw, name, model_path, flatten, img_res, cache, strict)

    reader = threading.Thread(target=_read_members, args=(img_path, q, stop, submit, bs, chunk, lo, hi, world),
                              name="rn-tar-reader", daemon=True)
    reader.start()
    try:
        items, done = [], False
        while not done:
            rec = q.get()
            if isinstance(rec, _Failure):
                raise rec.exc
            if rec is _END:
                done = True
            else:
                if world == 1 and rec.fut.result() is None:
                    continue                                     # unreadable image: skipped, every later index shifts
                items.append(rec)
                if len(items) < chunk:
                    continue
            n = len(items)
            if n == 0:
                break
            if n % bs == 0:
                for j in range(n // bs):
                    mine = items[j * bs + lo:j * bs + hi]
                    yield _batch([s.fut.result() for s in mine], [s.name for s in mine])
            else:
                # _pad_tail: np.repeat(a[:n], reps)[:bs] -- position p of the one batch holds sample p // reps
                reps = -(-bs // n)
                decoded = {}
                for i in sorted(set(p // reps for p in range(lo, hi))):
                    s = items[i]
                    decoded[i] = s.fut.result() if s.fut is not None else \
                        _decode_sample(s.raw, s.name, model_path, flatten, img_res, cache, True)
                picks = [p // reps for p in range(lo, hi)]
                yield _batch([decoded[i] for i in picks], [items[i].name for i in picks])
            items = []
    finally:
        stop.set()
        while True:                                              # unblock a reader waiting to put
            try:
                q.get_nowait()
            except queue.Empty:
                break
        reader.join()
        pool.shutdown(wait=True, cancel_futures=True)


def iter_host_batches(cfg, img_path, model_path, flatten, img_res, rank=0, world=1, workers=4, add_noise=False,
                      model_cache=256):
    """Per optimiser step, for rank `rank` of `world`: (images_u8 [b,res,res,Cs], voxels_u8 [b,64,64,64,1],
    poses_f32 [b,3], names) -- this rank's `parallel.shard_range(batch_size, rank, world)` of the batch that
    `data_loader(cfg, img_path, model_path, flatten=flatten, img_res=img_res)` followed by the script's
    `len(images) // batch_size` slices gives at that step (module docstring: chunks, tail rule).  The images are the decoded
    bytes with the file's own channel count Cs; `ops.target_u8_crop[_reference]` turns them into what the synchronous path
    feeds, bit for bit.

    Unreadable images.  world == 1: an image that fails to open or decode is skipped and every later index shifts,
    exactly as today.  world > 1: all ranks must agree on the sequence without decoding each other's pixels, so every
    rank opens the HEADER of every image member; a member whose header does not open is skipped on all ranks as today;
    a member whose header opens but whose pixels fail to decode raises on the rank that owns it, naming the member (the
    other ranks cannot know, and a desynchronised job would hang in the all-reduce instead).

    `workers` decode threads (1..16; an argument, never derived from the machine's CPU count).  `model_cache` bounds the
    LRU of decoded binvox models.  A batch whose members disagree on the channel count raises ValueError naming the
    member.  add_noise=True is refused: the reference's noise is host NumPy RNG added to float frames and has no uint8
    form.  Closing the generator (or dropping the last reference to it) stops and joins every thread it started."""
    if add_noise:
        raise ValueError("add_noise=True has no uint8 form (the noise is host NumPy RNG on float frames): use "
                         "tools.data_util.data_loader for noisy targets")
    workers = int(workers)
    if not 1 <= workers <= MAX_WORKERS:
        raise ValueError("workers=%d: expected 1..%d" % (workers, MAX_WORKERS))
    bs, bc = int(cfg['batch_size']), int(cfg['batches_chunk'])
    if bs < 1 or bc < 1:
        raise ValueError("batch_size=%d batches_chunk=%d" % (bs, bc))
    world, rank = int(world), int(rank)
    if world < 1 or not 0 <= rank < world or bs % world != 0:
        raise ValueError("rank %d of %d ranks for batch_size %d: every rank needs the same, non-empty shard" % (rank, world, bs))
    return _host_batches(cfg, img_path, model_path, bool(flatten), int(img_res), rank, world, workers, model_cache)


# -- device layer ----------------------------------------------------------------------------------------------------

class _Slot(object):
    """One pinned host buffer + one device buffer per stream of a batch, and the two events of the hand-over."""

    def __init__(self, torch, device, index, n_img, n_vox, n_pose):
        self.index = index
        self.pin = (torch.empty(n_img, dtype=torch.uint8, pin_memory=True), torch.empty(n_vox, dtype=torch.uint8, pin_memory=True),
                    torch.empty(n_pose, dtype=torch.float32, pin_memory=True))
        self.dev = tuple(torch.empty_like(p, device=device) for p in self.pin)
        self.filled = torch.cuda.Event()          # recorded on the side stream after the slot's copies
        self.released = torch.cuda.Event()        # recorded on the consumer's stream when it asks for the next batch


class _Shared(object):
    """What the producer thread and the loader share (the thread must not keep the loader itself alive)."""

    def __init__(self):
        self.stop = threading.Event()
        self.free = queue.Queue()                 # slot indices the consumer has released
        self.ready = queue.Queue()                # (slot, tensors, names) | _END | _Failure, in batch order


def _produce(shared, host_iter, device, depth):
    import torch
    side = None
    try:
        torch.cuda.set_device(device)
        side = torch.cuda.Stream(device)
        slots = None
        for images, voxels, poses, names in host_iter:
            arrays = (np.ascontiguousarray(images, np.uint8), np.ascontiguousarray(voxels, np.uint8),
                      np.ascontiguousarray(poses, np.float32))
            if slots is None:
                # allocated once; frames sized for four channels so that a later batch of RGBA files still fits
                b, res = arrays[0].shape[0], arrays[0].shape[1:3]
                slots = [_Slot(torch, device, k, b * res[0] * res[1] * 4, arrays[1].size, arrays[2].size) for k in range(depth)]
                for k in range(depth):
                    shared.free.put(k)
            k = _get(shared.free, shared.stop)
            if k is None:
                return
            slot = slots[k]
            slot.filled.synchronize()             # the pinned buffers' previous copy has left them
            views = []
            for a, pin, dev in zip(arrays, slot.pin, slot.dev):
                if a.size > pin.numel():
                    raise ValueError("batch of shape %s does not fit the slot sized by the first batch" % (a.shape,))
                pin[:a.size].copy_(torch.from_numpy(a).reshape(-1))
            with torch.cuda.stream(side):
                side.wait_event(slot.released)    # the consumer's work on the slot's previous batch is ahead of the overwrite
                for a, pin, dev in zip(arrays, slot.pin, slot.dev):
                    dev[:a.size].copy_(pin[:a.size], non_blocking=True)
                    views.append(dev[:a.size].view(a.shape))
                slot.filled.record(side)
            shared.ready.put((slot, tuple(views), names))
        shared.ready.put(_END)
    except BaseException as e:
        shared.ready.put(_Failure(e))
    finally:
        close = getattr(host_iter, "close", None)
        if close is not None:
            try:
                close()
            except Exception:
                pass
        if side is not None:
            side.synchronize()                    # no copy in flight into memory the allocator is about to get back


class PrefetchLoader(object):
    """Iterator (and context manager) over `host_iter` (iter_host_batches) yielding the same tuples as device tensors:
    (images uint8 [b,res,res,Cs], voxels uint8 [b,64,64,64,1], poses float32 [b,3], names).

    Slot protocol.  `depth` slots, each a pinned host buffer set and a device buffer set, allocated once.  The producer
    thread takes a released slot, waits (host side, in its own thread) for the slot's last copy event so the pinned
    buffers are free, fills them, and on ONE side stream waits for the slot's `released` event and enqueues the
    non-blocking copies followed by the slot's `filled` event.  `next()` first records `released` for the slot the consumer
    holds on the consumer's current stream -- everything the consumer enqueued on that batch is ahead of it -- then makes
    the current stream wait for the next slot's `filled` event.  The consumer never synchronises with the host; the
    tensors of a batch are valid until the next `next()`.

    An exception in the reader, a decode worker or the producer surfaces from `next()`.  Leaving the loop early, `close()`,
    the end of the `with` block and garbage collection all stop and join every thread; none outlives the loader.  Threads
    only: no process is started."""

    def __init__(self, host_iter, device, depth=2):
        import torch
        depth = int(depth)
        if not 1 <= depth <= 8:
            raise ValueError("depth=%d: expected 1..8 slots" % depth)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("PrefetchLoader feeds a HIP device; got %s" % self.device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._torch = torch
        self._shared = _Shared()
        self._held = None
        self._closed = False
        self._thread = threading.Thread(target=_produce, args=(self._shared, host_iter, self.device, depth),
                                        name="rn-prefetch", daemon=True)
        self._thread.start()

    def __iter__(self):
        return self

    def _release(self):
        if self._held is not None:
            self._held.released.record(self._torch.cuda.current_stream(self.device))
            self._shared.free.put(self._held.index)
            self._held = None

    def __next__(self):
        if self._closed:
            raise StopIteration
        self._release()
        item = self._shared.ready.get()
        if item is _END:
            self.close()
            raise StopIteration
        if isinstance(item, _Failure):
            self.close()
            raise item.exc
        slot, tensors, names = item
        self._torch.cuda.current_stream(self.device).wait_event(slot.filled)
        self._held = slot
        return tensors + (names,)

    next = __next__

    def close(self):
        """Stop the producer (and through it the host iterator's threads) and join it."""
        if self._closed:
            return
        self._closed = True
        self._held = None
        self._shared.stop.set()
        self._thread.join()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

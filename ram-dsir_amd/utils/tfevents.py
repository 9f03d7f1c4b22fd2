"""Minimal TensorBoard event-file writer for scalars, images and histograms: what the reference's `tensorboardX.SummaryWriter(save_path + '/log')`
produces for `writer.add_scalar(tag, value, iter_num)` (code/train.py:298-304, 467-473, 538) and `writer.add_image(tag, grid, iter_num)`
(train.py:306-329, 475-496).  tensorboardX / tensorboard are not installed here, so the three pieces are written out by hand:

  * TFRecord framing: uint64 length | masked crc32c(length) | payload | masked crc32c(payload), little endian;
  * crc32c (Castagnoli, reflected polynomial 0x82F63B78) with TensorFlow's mask ((crc >> 15 | crc << 17) + 0xa282ead8);
  * protobuf wire format of  Event { double wall_time = 1; int64 step = 2; string file_version = 3; Summary summary = 5; }
    Summary { repeated Value value = 1; }   Value { string tag = 1; float simple_value = 2; Image image = 4; HistogramProto histo = 5; }
    Image { int32 height = 1; int32 width = 2; int32 colorspace = 3; bytes encoded_image_string = 4; }
    HistogramProto { double min = 1; double max = 2; double num = 3; double sum = 4; double sum_squares = 5;
                     repeated double bucket_limit = 6 [packed]; repeated double bucket = 7 [packed]; }.

The first record of a file is Event{wall_time, file_version: "brain.Event:2"}; the file name follows TensorBoard's
`events.out.tfevents.<unix time>.<hostname>` pattern so that `tensorboard --logdir <save_path>/log` picks it up.
Image summaries take the finished uint8 HWC grid (train.py --tb_images composes it on the GPU: ramdsir/tb_images.py, which restates
make_grid and tensorboardX's float -> uint8 conversion) and encode it as PNG with Pillow, as tensorboardX does.  The checksum of such a
record (hundreds of kilobytes) goes through the HIP library's host routine rd_crc32c when the library is loadable; the pure-Python
loop below is the fallback and the reference of the tests.
Histogram summaries (train.py --tb_hist; no reference counterpart -- the reference writes scalars and images only) take finished
buckets under tensorboardX's add_histogram_raw: ramdsir/tb_hist.py counts them on the GPU and trims them on the writer thread.
"""
import io
import os
import socket
import struct
import time

_TABLE = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ 0x82F63B78 if _c & 1 else _c >> 1
    _TABLE.append(_c)


def crc32c(data, seed=0):
    """Pure Python; seed: the crc of the bytes in front of `data` (0 for none)."""
    c = seed ^ 0xFFFFFFFF
    for b in data:
        c = _TABLE[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


_native = None


def _native_crc32c():
    """rd_crc32c of the HIP library (host code), or False when the library cannot be loaded (not built, no ROCm runtime)."""
    global _native
    if _native is None:
        try:
            from ramdsir import _lib
            _native = _lib.lib().rd_crc32c
        except Exception:
            _native = False
    return _native


def crc32c_fast(data, seed=0):
    """crc32c(data) through rd_crc32c when available (seed: the crc of the bytes in front), else the Python loop."""
    fn = _native_crc32c() if len(data) >= 64 else None          # (a ctypes call costs more than 64 table steps)
    return fn(bytes(data), len(data), seed) if fn else crc32c(data, seed)


def masked_crc(data):
    c = crc32c_fast(data)
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def _varint(n):
    n &= (1 << 64) - 1                     # int64 fields: two's complement, ten bytes when negative
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        if n:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _key(field, wire):
    return _varint((field << 3) | wire)


def _bytes_field(field, payload):
    return _key(field, 2) + _varint(len(payload)) + payload


def encode_png(img_hwc_uint8):
    """PNG bytes of a uint8 (H, W, 3) / (H, W, 1) / (H, W) array (Pillow, as tensorboardX's make_image)."""
    import numpy as np
    from PIL import Image
    a = np.ascontiguousarray(img_hwc_uint8)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3)):
        raise ValueError('add_image takes a uint8 HWC array with 1 or 3 channels, got %s %s' % (a.dtype, a.shape))
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format='PNG')
    return a.shape[0], a.shape[1], (3 if a.ndim == 3 else 1), buf.getvalue()


def encode_histo(mn, mx, num, total, sum_squares, bucket_limits, bucket_counts):
    """The bytes of one HistogramProto: five doubles, then the limits and the counts as packed repeated doubles."""
    limits, counts = [float(v) for v in bucket_limits], [float(v) for v in bucket_counts]
    if len(limits) != len(counts):
        raise ValueError('a histogram has one count per limit, got %d limits and %d counts' % (len(limits), len(counts)))
    h = b''.join(_key(f, 1) + struct.pack('<d', float(v)) for f, v in enumerate((mn, mx, num, total, sum_squares), 1))
    return h + _bytes_field(6, struct.pack('<%dd' % len(limits), *limits)) + _bytes_field(7, struct.pack('<%dd' % len(counts), *counts))


def encode_event(wall_time, step=None, file_version=None, scalars=None, images=None, histos=None):
    """scalars: list of (tag, float); images: list of (tag, height, width, colorspace, png bytes); histos: list of (tag, min, max, num,
    sum, sum_squares, bucket limits, bucket counts)."""
    ev = _key(1, 1) + struct.pack('<d', wall_time)
    if step is not None:
        ev += _key(2, 0) + _varint(int(step))
    if file_version is not None:
        ev += _bytes_field(3, file_version.encode())
    if scalars:
        summ = b''
        for tag, v in scalars:
            val = _bytes_field(1, tag.encode()) + _key(2, 5) + struct.pack('<f', float(v))
            summ += _bytes_field(1, val)
        ev += _bytes_field(5, summ)
    if images:
        summ = b''
        for tag, h, w, cs, png in images:
            im = _key(1, 0) + _varint(h) + _key(2, 0) + _varint(w) + _key(3, 0) + _varint(cs) + _bytes_field(4, bytes(png))
            summ += _bytes_field(1, _bytes_field(1, tag.encode()) + _bytes_field(4, im))
        ev += _bytes_field(5, summ)
    if histos:
        summ = b''
        for h in histos:
            summ += _bytes_field(1, _bytes_field(1, h[0].encode()) + _bytes_field(5, encode_histo(*h[1:])))
        ev += _bytes_field(5, summ)
    return ev


def frame(payload):
    head = struct.pack('<Q', len(payload))
    return head + struct.pack('<I', masked_crc(head)) + payload + struct.pack('<I', masked_crc(payload))


class SummaryWriter(object):
    """`add_scalar(tag, scalar_value, global_step)` / `add_image(tag, img, global_step)` / `flush()` / `close()` of
    tensorboardX.SummaryWriter (add_image with dataformats='HWC' and a finished uint8 image)."""

    def __init__(self, logdir, flush_secs=30):
        os.makedirs(logdir, exist_ok=True)
        self.logdir = logdir
        self.path = os.path.join(logdir, 'events.out.tfevents.%010d.%s' % (int(time.time()), socket.gethostname()))
        self._f = open(self.path, 'wb')
        self._f.write(frame(encode_event(time.time(), file_version='brain.Event:2')))
        self._flush_secs, self._last = flush_secs, time.time()

    def add_scalar(self, tag, scalar_value, global_step=None, walltime=None):
        self.add_scalars_at(global_step, [(tag, scalar_value)], walltime)

    def add_scalars_at(self, global_step, pairs, walltime=None):
        """Several scalars of one step, one record each (as consecutive add_scalar calls write them)."""
        t = time.time() if walltime is None else walltime
        for tag, v in pairs:
            self._f.write(frame(encode_event(t, step=global_step, scalars=[(tag, v)])))
        if t - self._last > self._flush_secs:
            self.flush()

    def add_image(self, tag, img_hwc_uint8, global_step=None, walltime=None):
        """One Summary.Value{tag, image} record: the uint8 HWC array as PNG."""
        t = time.time() if walltime is None else walltime
        self._f.write(frame(encode_event(t, step=global_step, images=[(tag,) + encode_png(img_hwc_uint8)])))
        if t - self._last > self._flush_secs:
            self.flush()

    def add_histogram_raw(self, tag, min, max, num, sum, sum_squares, bucket_limits, bucket_counts, global_step=None, walltime=None):
        """One Summary.Value{tag, histo} record from finished buckets (tensorboardX's name and argument order): bucket_counts[i] values
        lie in the bucket whose upper edge is bucket_limits[i]."""
        t = time.time() if walltime is None else walltime
        self._f.write(frame(encode_event(t, step=global_step, histos=[(tag, min, max, num, sum, sum_squares, bucket_limits, bucket_counts)])))
        if t - self._last > self._flush_secs:
            self.flush()

    def flush(self):
        self._f.flush()
        self._last = time.time()

    def close(self):
        if not self._f.closed:
            self._f.flush()
            self._f.close()


class QueuedWriter(SummaryWriter):
    """A SummaryWriter whose records are encoded and written by ONE thread that owns the file (train.py --tb_images / --tb_hist): the training
    thread only enqueues.  add_scalars_at takes its wall time at the call, as the direct writer does; add_images_at(step, fetch)
    takes a callable that returns [(tag, uint8 HWC array)] when the data has arrived (ramdsir.tb_images.Pending: it waits for the
    event behind the device-to-host copy) -- PNG encoding (zlib, Pillow: both release the GIL), checksums and the write happen in the
    thread.  add_histograms_at(step, fetch) is the third kind of item: fetch() returns (histograms, scalars) -- [(tag, min, max, num,
    sum, sum_squares, bucket limits, bucket counts)] and [(tag, value)] -- when the data has arrived (ramdsir.tb_hist.Pending), written
    as one record each, the histograms first.  Records appear in the order of the calls.  close() drains the queue; an error in the
    thread is raised there."""

    def __init__(self, logdir, flush_secs=30):
        import queue
        import threading
        SummaryWriter.__init__(self, logdir, flush_secs)
        self._q, self._err = queue.Queue(), None
        self.seconds = dict(wait=0.0, png=0.0, crc=0.0, write=0.0, records=0, calls=0)      # host time of the image records (profiles/tb_images.md)
        self.seconds['histo'] = dict(wait=0.0, encode=0.0, write=0.0, records=0, calls=0)  # ... and of the histogram records (profiles/tb_hist.md)
        self._t = threading.Thread(target=self._drain, name='tfevents-writer', daemon=True)
        self._t.start()

    def add_scalars_at(self, global_step, pairs, walltime=None):
        self._q.put(('scalars', global_step, list(pairs), time.time() if walltime is None else walltime))

    def add_images_at(self, global_step, fetch, walltime=None):
        self._q.put(('images', global_step, fetch, time.time() if walltime is None else walltime))

    def add_image(self, tag, img_hwc_uint8, global_step=None, walltime=None):
        self.add_images_at(global_step, lambda: [(tag, img_hwc_uint8)], walltime)

    def add_histograms_at(self, global_step, fetch, walltime=None):
        self._q.put(('histos', global_step, fetch, time.time() if walltime is None else walltime))

    def add_histogram_raw(self, tag, min, max, num, sum, sum_squares, bucket_limits, bucket_counts, global_step=None, walltime=None):
        h = (tag, min, max, num, sum, sum_squares, list(bucket_limits), list(bucket_counts))
        self.add_histograms_at(global_step, lambda: ([h], []), walltime)

    def _write_histos(self, step, fetch, t):
        sec = self.seconds['histo']
        t0 = time.perf_counter()
        histos, scalars = fetch()
        t1 = time.perf_counter()
        recs = [frame(encode_event(t, step=step, histos=[h])) for h in histos]
        recs += [frame(encode_event(t, step=step, scalars=[p])) for p in scalars]
        t2 = time.perf_counter()
        self._f.write(b''.join(recs))
        t3 = time.perf_counter()
        sec['wait'] += t1 - t0                      # the copy's event and the trimming (ramdsir.tb_hist.Pending.fetch)
        sec['encode'] += t2 - t1                    # protobuf, crc32c, framing
        sec['write'] += t3 - t2
        sec['records'] += len(recs)
        sec['calls'] += 1

    def _drain(self):
        while True:
            item = self._q.get()
            if item is None:
                return
            if self._err is not None:
                continue                    # keep consuming so that close() never blocks
            try:
                kind, step, payload, t = item
                if kind == 'scalars':
                    SummaryWriter.add_scalars_at(self, step, payload, t)
                    continue
                if kind == 'histos':
                    self._write_histos(step, payload, t)
                    if t - self._last > self._flush_secs:
                        self.flush()
                    continue
                sec = self.seconds
                t0 = time.perf_counter()
                images = payload()
                t1 = time.perf_counter()
                sec['wait'] += t1 - t0
                sec['calls'] += 1
                for tag, img in images:
                    t1 = time.perf_counter()
                    ev = encode_event(t, step=step, images=[(tag,) + encode_png(img)])
                    t2 = time.perf_counter()                 # (the protobuf wrapping counts as PNG time: a few byte joins)
                    rec = frame(ev)
                    t3 = time.perf_counter()
                    self._f.write(rec)
                    t4 = time.perf_counter()
                    sec['png'] += t2 - t1
                    sec['crc'] += t3 - t2
                    sec['write'] += t4 - t3
                    sec['records'] += 1
                if t - self._last > self._flush_secs:
                    self.flush()
            except Exception as e:          # noqa: BLE001 -- reported by close()
                self._err = e

    def close(self):
        if self._t.is_alive():
            self._q.put(None)
            self._t.join()
        SummaryWriter.close(self)
        if self._err is not None:
            err, self._err = self._err, None
            raise err


# ---------------------------------------------------------------------------------------------- reader (tests, tooling)
def _read_varint(buf, pos):
    shift = n = 0
    while True:
        b = buf[pos]
        pos += 1
        n |= (b & 0x7F) << shift
        if not b & 0x80:
            return n, pos
        shift += 7


def _fields(buf):
    pos = 0
    while pos < len(buf):
        k, pos = _read_varint(buf, pos)
        field, wire = k >> 3, k & 7
        if wire == 0:
            v, pos = _read_varint(buf, pos)
        elif wire == 1:
            v, pos = buf[pos:pos + 8], pos + 8
        elif wire == 5:
            v, pos = buf[pos:pos + 4], pos + 4
        elif wire == 2:
            n, pos = _read_varint(buf, pos)
            v, pos = buf[pos:pos + n], pos + n
        else:
            raise ValueError('wire type %d' % wire)
        yield field, wire, v


def read_events(path):
    """-> list of dicts {wall_time, step, file_version, scalars: [(tag, value)], images: [(tag, height, width, colorspace, png bytes)],
    histos: [(tag, min, max, num, sum, sum_squares, bucket limits, bucket counts)] (the last two as tuples of floats)}; every CRC is
    verified."""
    out = []
    with open(path, 'rb') as f:
        data = f.read()
    pos = 0
    while pos < len(data):
        head = data[pos:pos + 8]
        (n,) = struct.unpack('<Q', head)
        (c1,) = struct.unpack('<I', data[pos + 8:pos + 12])
        payload = data[pos + 12:pos + 12 + n]
        (c2,) = struct.unpack('<I', data[pos + 12 + n:pos + 16 + n])
        if c1 != masked_crc(head) or c2 != masked_crc(payload) or len(payload) != n:
            raise ValueError('corrupt record at byte %d' % pos)
        pos += 16 + n
        ev = dict(wall_time=None, step=0, file_version=None, scalars=[], images=[], histos=[])
        for field, wire, v in _fields(payload):
            if field == 1:
                ev['wall_time'] = struct.unpack('<d', v)[0]
            elif field == 2:
                ev['step'] = v - (1 << 64) if v >> 63 else v
            elif field == 3:
                ev['file_version'] = v.decode()
            elif field == 5:
                for f1, _, val in _fields(v):
                    if f1 != 1:
                        continue
                    tag, sv, im, hi = None, None, None, None
                    for f2, _, x in _fields(val):
                        if f2 == 1:
                            tag = x.decode()
                        elif f2 == 2:
                            sv = struct.unpack('<f', x)[0]
                        elif f2 == 4:
                            im = {f3: y for f3, _, y in _fields(x)}
                        elif f2 == 5:
                            hi = {f3: y for f3, _, y in _fields(x)}
                    if hi is not None:
                        five = [struct.unpack('<d', hi[k])[0] if k in hi else 0.0 for k in range(1, 6)]
                        packed = [struct.unpack('<%dd' % (len(hi.get(k, b'')) // 8), hi.get(k, b'')) for k in (6, 7)]
                        ev['histos'].append((tag,) + tuple(five) + tuple(packed))
                    elif im is not None:
                        ev['images'].append((tag, im.get(1, 0), im.get(2, 0), im.get(3, 0), bytes(im.get(4, b''))))
                    else:
                        ev['scalars'].append((tag, sv))
        out.append(ev)
    return out

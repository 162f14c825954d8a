"""input_fn of the ACR module: acr_module/acr/acr_datasets.py without TensorFlow.

``prepare_dataset`` keeps the reference's semantics (:9-43 parse_sequence_example, :74-123 make_dataset, :145-164 prepare_dataset):
GZIP TFRecord files of tf.train.SequenceExample read in the given order, ``text[:truncate_tokens_length]``, batches of ``batch_size``
zero-padded to the batch's longest text (the last batch of the stream may be partial), single features squeezed to [B], the label
features split off (and, as in the reference, still present among the features), the batch sequence repeated ``epochs`` times and
then shuffled BY BATCH through a buffer of ``shuffle_buffer_size`` batches.

The shuffle is tf.data's buffer algorithm (fill the buffer, draw one slot uniformly, refill it from the stream) on a numpy
RandomState(seed): the same seed gives the same order; TensorFlow's own random stream is not reproduced.

Records come from the C++ codec's raw record stream (cham_tfr_next: framing, CRC, gzip); the SequenceExample protobuf of a record is
decoded here.  There is no label shift and no required feature (the session reader of the NAR module has both)."""
import ctypes
import struct

import numpy as np

from .. import _tfrecord
from .._tfrecord import check

RANDOM_SEED = 42


def _varint(buf, i):
    r, s = 0, 0
    while True:
        b = buf[i]; i += 1
        r |= (b & 0x7F) << s
        if b < 0x80:
            return r, i
        s += 7
        if s > 63:
            raise _tfrecord.TFRecordError("malformed SequenceExample protobuf (varint)")


def _fields(buf):
    """(field number, wire type, value) of one message; value = int (varint) or bytes (length-delimited / fixed)."""
    i, n = 0, len(buf)
    while i < n:
        key, i = _varint(buf, i)
        wt = key & 7
        if wt == 0:
            v, i = _varint(buf, i)
        elif wt == 2:
            ln, i = _varint(buf, i)
            if i + ln > n:
                raise _tfrecord.TFRecordError("malformed SequenceExample protobuf (length)")
            v = buf[i:i + ln]; i += ln
        elif wt == 5:
            v = buf[i:i + 4]; i += 4
        elif wt == 1:
            v = buf[i:i + 8]; i += 8
        else:
            raise _tfrecord.TFRecordError("malformed SequenceExample protobuf (wire type %d)" % wt)
        yield key >> 3, wt, v


def _signed(v):
    return v - (1 << 64) if v >= (1 << 63) else v


def _feature_values(buf):
    """tf.train.Feature -> list of values (bytes_list = 1, float_list = 2, int64_list = 3; packed or not)."""
    out = []
    for no, _, lst in _fields(buf):
        for _, wt, v in _fields(lst):
            if no == 3:
                if wt == 0:
                    out.append(_signed(v))
                else:
                    i = 0
                    while i < len(v):
                        x, i = _varint(v, i)
                        out.append(_signed(x))
            elif no == 2:
                out.extend(struct.unpack("<%df" % (len(v) // 4), v))
            else:
                out.append(bytes(v))
    return out


def _map_entries(buf):
    """map<string, X> entries of Features / FeatureLists (field 1; key = 1, value = 2) -> {name: raw value bytes}."""
    out = {}
    for no, _, entry in _fields(buf):
        if no != 1:
            continue
        k, v = None, b""
        for eno, _, ev in _fields(entry):
            if eno == 1:
                k = bytes(ev).decode()
            elif eno == 2:
                v = ev
        out[k] = v
    return out


def parse_sequence_example(record, features_config, truncate_sequence_length=300):
    """acr_datasets.py:9-43: {single feature: scalar, sequence feature: 1-D list}; 'text' truncated to its first N tokens."""
    ctx, seq = {}, {}
    for no, _, v in _fields(record):
        if no == 1:
            ctx = _map_entries(v)
        elif no == 2:
            seq = _map_entries(v)
    out = {}
    for name in features_config['single_features']:
        vals = _feature_values(ctx[name]) if name in ctx else []
        if len(vals) != 1:
            raise _tfrecord.TFRecordError("context feature %r is missing or not a scalar" % name)
        out[name] = vals[0]
    for name in features_config['sequence_features']:
        if name not in seq:
            raise _tfrecord.TFRecordError("sequence feature %r is missing" % name)
        steps = []
        for no, _, feat in _fields(seq[name]):
            if no == 1:
                steps.extend(_feature_values(feat))
        out[name] = steps
    out['text'] = out['text'][:truncate_sequence_length]
    return out


def read_records(path, check_crc=True):
    """Raw records of one GZIP TFRecord file (tf.data.TFRecordDataset(path, 'GZIP'))."""
    lib = _tfrecord.load()
    h = lib.cham_tfr_open(path.encode())
    if not h:
        raise _tfrecord.TFRecordError("cannot open %s" % path)
    try:
        data, ln = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
        while True:
            rc = check(lib.cham_tfr_next(h, ctypes.byref(data), ctypes.byref(ln), 1 if check_crc else 0), "cham_tfr_next(%s)" % path)
            if rc == _tfrecord.EOF:
                return
            yield ctypes.string_at(data, ln.value)
    finally:
        lib.cham_tfr_close(h)


def _np_dtype(cfg):
    return np.float32 if cfg['dtype'] == 'float' else np.int64


def make_batches(files, features_config, batch_size=128, truncate_sequence_length=300):
    """acr_datasets.py:74-123 make_dataset as a generator of (features, labels)."""
    if isinstance(files, str):
        files = [files]
    single, seqf = features_config['single_features'], features_config['sequence_features']

    def emit(rows):
        feats = {n: np.asarray([r[n] for r in rows], dtype=_np_dtype(single[n])) for n in single}
        for n in seqf:
            L = max(len(r[n]) for r in rows)
            a = np.zeros((len(rows), L), dtype=_np_dtype(seqf[n]))
            for i, r in enumerate(rows):
                a[i, :len(r[n])] = r[n]
            feats[n] = a
        labels = {n: feats[n] for n in feats if n in features_config['label_features']}
        return feats, labels

    rows = []
    for f in files:
        for rec in read_records(f):
            rows.append(parse_sequence_example(rec, features_config, truncate_sequence_length))
            if len(rows) == batch_size:
                yield emit(rows)
                rows = []
    if rows:
        yield emit(rows)


def _shuffle(stream, buffer_size, rng):
    buf = []
    for x in stream:
        if len(buf) < buffer_size:
            buf.append(x)
            continue
        i = rng.randint(len(buf))
        yield buf[i]
        buf[i] = x
    while buf:
        i = rng.randint(len(buf))
        yield buf[i]
        buf[i] = buf[-1]
        buf.pop()


class ArticleDataset:
    """The one-shot iterator of acr_datasets.py:145-164: iterate once, get (features, labels) numpy batches."""

    def __init__(self, files, features_config, batch_size, epochs, shuffle_dataset, shuffle_buffer_size, truncate_tokens_length, seed):
        self._args = (files, features_config, batch_size, truncate_tokens_length)
        self.epochs, self.shuffle_dataset, self.shuffle_buffer_size, self.seed = epochs, shuffle_dataset, shuffle_buffer_size, seed

    def _repeated(self):
        cache = [] if self.epochs > 1 else None          # decoded once, replayed for the later epochs
        for b in make_batches(*self._args):
            if cache is not None:
                cache.append(b)
            yield b
        for _ in range(1, self.epochs):
            for b in cache:
                yield b

    def __iter__(self):
        stream = self._repeated()
        if self.shuffle_dataset:
            stream = _shuffle(stream, max(1, int(self.shuffle_buffer_size)), np.random.RandomState(self.seed))
        return stream


def prepare_dataset(files, features_config, batch_size=128, epochs=1, shuffle_dataset=True, shuffle_buffer_size=3000,
                    truncate_tokens_length=300, seed=RANDOM_SEED):
    """acr_datasets.py:145-164 (``seed``: the batch shuffle's numpy RandomState, see the module docstring)."""
    return ArticleDataset(files, features_config, batch_size, epochs, shuffle_dataset, shuffle_buffer_size, truncate_tokens_length, seed)

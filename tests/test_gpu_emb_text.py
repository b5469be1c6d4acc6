"""The embedding text kernels (csrc/dw_embtext.hip) against the host path, which
tests/test_emb_text.py pins to the numpy / CPython reference: the same bytes, the same line
offsets, for the smallest shapes at which the kernels take another path — one value, a ragged
last tile (d = 3, 127, 129), the two LDS line sizes (d <= 128, d <= 512), several blocks
(n = 65, 257), every alignment of a line's start, a misaligned table."""
import ctypes

import numpy as np
import pytest
import torch

import embtext_ref as ref
from shallow_encoders import _native
from shallow_encoders.word2vec.embeddings_io import f32text_table, save_word2vec_format

pytestmark = pytest.mark.gpu

CANARY = 64


def _hard_table(n, d, finite=False):
    bits = ref.hard_bits()
    if finite:
        bits = bits[(bits & 0x7F800000) != 0x7F800000]
    reps = -(-n * d // len(bits))
    return np.tile(bits, reps)[:n * d].view(np.float32).reshape(n, d).copy()


class Dev:
    """One table on the device with its keys; sizes() and write() call the two passes raw."""

    def __init__(self, dev, table, rows=None, keys_i64=None, key_strs=None, table_t=None):
        self.dev = dev
        self.t = torch.from_numpy(table).to(dev) if table_t is None else table_t
        self.V, self.d = self.t.shape
        self.rows = None if rows is None else torch.as_tensor(rows, dtype=torch.int64).to(dev)
        self.n = self.V if rows is None else len(rows)
        self.k64 = self.kb = self.ko = None
        if key_strs is not None:
            enc = [k.encode('utf-8') for k in key_strs]
            off = np.zeros(self.n + 1, dtype=np.int64)
            np.cumsum([len(e) for e in enc], out=off[1:])
            self.kb = torch.from_numpy(np.frombuffer(b''.join(enc), dtype=np.uint8).copy()).to(dev)
            self.ko = torch.from_numpy(off).to(dev)
        else:
            k = np.arange(self.n, dtype=np.int64) if keys_i64 is None else keys_i64
            self.k64 = torch.as_tensor(k, dtype=torch.int64).to(dev)
        self.tab = f32text_table(dev)
        self.line_off = torch.empty(self.n + 1, dtype=torch.int64, device=dev)

    def _ins(self, d=None):
        p = _native.ptr
        return (self.t.data_ptr(), self.V, self.d if d is None else d, p(self.rows), self.n,
                p(self.k64), p(self.kb), p(self.ko), self.tab.data_ptr())

    def sizes(self):
        """(line_off on the host, status)."""
        status = torch.zeros(1, dtype=torch.int32, device=self.dev)
        nb = ctypes.c_size_t(0)
        _native.call('dw_embtext_workspace_bytes', self.n, self.d, ctypes.byref(nb))
        ws = torch.empty(max(1, nb.value), dtype=torch.uint8, device=self.dev)
        _native.call('dw_embtext_sizes', *self._ins(), self.line_off.data_ptr(),
                     status.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream(self.dev))
        return self.line_off.cpu().numpy(), int(status.item())

    def write(self, r0, r1, size, short=0, shift=0):
        """(the buffer's first `size` bytes, the canary behind them intact?, status): rows
        [r0, r1) into a buffer of capacity size - short that starts `shift` bytes behind a
        16-byte boundary, with CANARY bytes of 0xA5 behind `size`."""
        buf = torch.full((shift + size + CANARY,), 0xA5, dtype=torch.uint8, device=self.dev)
        assert buf.data_ptr() % 16 == 0
        status = torch.zeros(1, dtype=torch.int32, device=self.dev)
        _native.call('dw_embtext_write', *self._ins(), self.line_off.data_ptr(), r0, r1,
                     buf.data_ptr() + shift, size - short, status.data_ptr(),
                     _native.stream(self.dev))
        got = buf.cpu().numpy()
        ok = bool((got[:shift] == 0xA5).all() and (got[shift + size:] == 0xA5).all())
        return got[shift:shift + size].tobytes(), ok, int(status.item())


SHAPES = [(1, 1), (3, 2), (65, 3), (64, 64), (5, 127), (7, 128), (3, 129), (2, 512), (257, 16)]


@pytest.mark.parametrize('n,d', SHAPES)
def test_device_bytes_equal_the_host_path(hip_device, n, d):
    table = _hard_table(n, d)
    want, want_off, want_st = ref.host_lines(table)
    dv = Dev(hip_device, table)
    off, st = dv.sizes()
    np.testing.assert_array_equal(off, want_off)
    assert st == want_st == (0 if np.isfinite(table).all() else _native.DW_S_NONFINITE)
    got, ok, wst = dv.write(0, n, len(want))
    assert got == want and ok and wst == 0
    if n * d <= 4096:   # and the reference itself, line by line
        body = ref.file_bytes(range(n), table).split(b'\n', 1)[1]
        assert got == body
        lens = [len(ln) + 1 for ln in body.split(b'\n')[:-1]]
        np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum(lens)]))
    again, ok, _ = dv.write(0, n, len(want), shift=5)    # rerun, another buffer alignment
    assert again == want and ok


def test_random_bit_patterns(hip_device):
    rng = np.random.default_rng(11)
    table = rng.integers(0, 1 << 32, size=(8192, 128), dtype=np.uint64).astype(np.uint32) \
        .view(np.float32)
    assert not np.isfinite(table).all()
    want, want_off, want_st = ref.host_lines(table)
    dv = Dev(hip_device, table)
    off, st = dv.sizes()
    np.testing.assert_array_equal(off, want_off)
    assert st == want_st == _native.DW_S_NONFINITE
    got, ok, wst = dv.write(0, 8192, len(want))
    assert got == want and ok and wst == 0


def test_misaligned_table_rows_and_key_forms(hip_device):
    n, d = 33, 21
    table = _hard_table(n, d, finite=True)
    want, want_off, _ = ref.host_lines(table)
    flat = torch.zeros(n * d + 1, dtype=torch.float32, device=hip_device)
    flat[1:] = torch.from_numpy(table).to(hip_device).reshape(-1)
    shifted = flat[1:].view(n, d)
    assert shifted.data_ptr() % 16 == 4
    outs = []
    for dv in (Dev(hip_device, table, table_t=shifted),
               Dev(hip_device, table, rows=np.arange(n)),
               Dev(hip_device, table, key_strs=[str(i) for i in range(n)]),
               Dev(hip_device, table, rows=np.arange(n), key_strs=[str(i) for i in range(n)])):
        off, st = dv.sizes()
        np.testing.assert_array_equal(off, want_off)
        assert st == 0
        outs.append(dv.write(0, n, len(want)))
    assert all(o == (want, True, 0) for o in outs)
    # rows as a permutation with repeats, multibyte keys, int64 keys up to 10^18 - 1
    rows = np.asarray([32, 0, 5, 5, 17, 32, 1], dtype=np.int64)
    names = [f'nœud{i}√' for i in range(len(rows))]
    want, want_off, _ = ref.host_lines(table, rows=rows, key_strs=names)
    dv = Dev(hip_device, table, rows=rows, key_strs=names)
    np.testing.assert_array_equal(dv.sizes()[0], want_off)
    assert dv.write(0, len(rows), len(want)) == (want, True, 0)
    ids = np.asarray([0, 10 ** 18 - 1, 7, 10, 99, 100, 12345678901], dtype=np.int64)
    want, want_off, _ = ref.host_lines(table, rows=rows, keys_i64=ids)
    dv = Dev(hip_device, table, rows=rows, keys_i64=ids)
    np.testing.assert_array_equal(dv.sizes()[0], want_off)
    assert dv.write(0, len(rows), len(want)) == (want, True, 0)


def test_row_ranges_canary_and_capacity(hip_device):
    n, d = 65, 3
    table = _hard_table(n, d, finite=True)
    whole, off, _ = ref.host_lines(table)
    dv = Dev(hip_device, table)
    np.testing.assert_array_equal(dv.sizes()[0], off)
    for cut in range(n + 1):
        a, ok_a, st_a = dv.write(0, cut, int(off[cut]))
        b, ok_b, st_b = dv.write(cut, n, int(off[n] - off[cut]), shift=cut % 16)
        assert a + b == whole and ok_a and ok_b and st_a == 0 and st_b == 0, cut
    # one byte short: nothing is written, the condition is reported
    for r0, r1 in ((0, n), (7, 8), (30, 65)):
        size = int(off[r1] - off[r0])
        got, ok, st = dv.write(r0, r1, size, short=1)
        assert got == b'\xa5' * size and ok and st == _native.DW_S_RECORDS_FULL


def test_status_bits(hip_device):
    table = _hard_table(9, 4, finite=True)
    assert Dev(hip_device, table).sizes()[1] == 0
    for rows in ([0, 9], [-1, 3], [1 << 40]):
        dv = Dev(hip_device, table, rows=np.asarray(rows, dtype=np.int64))
        off, st = dv.sizes()
        want, want_off, want_st = ref.host_lines(table, rows=np.asarray(rows, dtype=np.int64))
        assert st == want_st == _native.DW_S_BAD_INDEX
        np.testing.assert_array_equal(off, want_off)
        assert dv.write(0, len(rows), len(want))[:2] == (want, True)   # a bad row prints zeros
    keys = np.arange(9, dtype=np.int64)
    keys[4] = -5
    assert Dev(hip_device, table, keys_i64=keys).sizes()[1] == _native.DW_S_BAD_INDEX
    for v in (np.nan, np.inf, -np.inf):
        t = table.copy()
        t[8, 3] = v
        assert Dev(hip_device, t).sizes()[1] == _native.DW_S_NONFINITE
        assert Dev(hip_device, t, rows=np.arange(8)).sizes()[1] == 0
    t[0, 0] = np.nan
    dv = Dev(hip_device, t, rows=np.asarray([0, 12], dtype=np.int64))
    assert dv.sizes()[1] == _native.DW_S_NONFINITE | _native.DW_S_BAD_INDEX


def test_dim_513_is_refused_before_any_launch(hip_device):
    lib = _native.load()
    dv = Dev(hip_device, _hard_table(2, 8))
    status = torch.zeros(1, dtype=torch.int32, device=hip_device)
    rc = lib.dw_embtext_sizes(*dv._ins(d=513), dv.line_off.data_ptr(), status.data_ptr(),
                              status.data_ptr(), 4, _native.stream(hip_device))
    assert rc == _native.DW_E_UNSUPPORTED and b'dim 513 > 512' in lib.dw_last_error_string()
    rc = lib.dw_embtext_write(*dv._ins(d=513), dv.line_off.data_ptr(), 0, 2, status.data_ptr(),
                              4, status.data_ptr(), _native.stream(hip_device))
    assert rc == _native.DW_E_UNSUPPORTED and b'dim 513 > 512' in lib.dw_last_error_string()
    torch.cuda.synchronize()
    assert int(status.item()) == 0


def test_save_on_a_device_tensor_equals_the_host_file(hip_device, tmp_path):
    table = _hard_table(300, 17, finite=True)
    rows = np.random.default_rng(2).integers(1, 300, size=500)
    names = [f'v{i}' for i in range(len(rows))]
    host, devp = str(tmp_path / 'h.emb'), str(tmp_path / 'd.emb')
    t = torch.from_numpy(table)
    n_host = save_word2vec_format(host, t, keys=names, rows=rows)
    want = open(host, 'rb').read()
    assert n_host == len(want)
    for chunk in (1, 700, 5000, 256 << 20):   # < a line, a few lines, many chunks, one chunk
        n_dev = save_word2vec_format(devp, t.to(hip_device), keys=names, rows=rows,
                                     chunk_bytes=chunk)
        assert open(devp, 'rb').read() == want and n_dev == n_host, chunk
    bad = table.copy()
    bad[7, 2] = np.nan
    import os
    os.remove(devp)
    with pytest.raises(ValueError, match='row 7, column 2'):
        save_word2vec_format(devp, torch.from_numpy(bad).to(hip_device))
    assert not os.path.exists(devp)
    with pytest.raises(IndexError):
        save_word2vec_format(devp, t.to(hip_device), rows=[0, 300])
    save_word2vec_format(devp, torch.from_numpy(bad).to(hip_device), nonfinite='write')
    save_word2vec_format(host, bad, nonfinite='write')
    assert open(devp, 'rb').read() == open(host, 'rb').read()

"""audio.read / to_mono on seeded files written here in every container and coding the reference's recipes need (RIFF WAV PCM
8/16/24/32-bit, IEEE float 32/64, WAVE_FORMAT_EXTENSIBLE, NIST SPHERE both byte orders): exact equality with the libsndfile
float32 conversions; the 16-kHz 16-bit files give exactly what the previous 16-kHz-only loader gave."""
import struct
import wave

import numpy as np
import pytest

from phones_las_amd import audio

GUID_TAIL = b'\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71'


def _wav(path, payload, tag, channels, sr, bits, extra_chunks=(), extensible=False, data_size=None):
    width = (bits + 7) // 8
    block = channels * width
    if extensible:
        fmt = struct.pack('<HHIIHHHHI', 0xFFFE, channels, sr, sr * block, block, bits, 22, bits, 0) + struct.pack('<H', tag) + GUID_TAIL
    else:
        fmt = struct.pack('<HHIIHH', tag, channels, sr, sr * block, block, bits)
    chunks = [(b'fmt ', fmt)] + list(extra_chunks)
    body = b''
    for cid, c in chunks:
        body += cid + struct.pack('<I', len(c)) + c + (b'\x00' if len(c) & 1 else b'')
    body += b'data' + struct.pack('<I', len(payload) if data_size is None else data_size) + payload
    with open(path, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', 4 + len(body)) + b'WAVE' + body)


def _sphere(path, payload, sr, channels, nbytes, order, coding='pcm', header_size=1024, count=None):
    fields = ['sample_count -i %d' % (count if count is not None else len(payload) // (nbytes * channels)),
              'sample_rate -i %d' % sr, 'channel_count -i %d' % channels, 'sample_n_bytes -i %d' % nbytes,
              'sample_byte_format -s%d %s' % (len(order), order), 'sample_coding -s%d %s' % (len(coding), coding),
              'sample_sig_bits -i %d' % (8 * nbytes), 'database_id -s5 TIMIT', 'end_head']
    head = ('NIST_1A\n   %d\n' % header_size + '\n'.join(fields) + '\n').encode()
    head += b' ' * (header_size - len(head))
    with open(path, 'wb') as f:
        f.write(head + payload)


def _ints(rng, n, bits):
    return rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), size=n, dtype=np.int64)


def _i24_bytes(s, big=False):
    u = (s & 0xFFFFFF).astype(np.uint32)
    b = np.stack([(u >> 0) & 255, (u >> 8) & 255, (u >> 16) & 255], 1).astype(np.uint8)
    return (b[:, ::-1] if big else b).tobytes()


def _frames(flat, channels):
    return flat if channels == 1 else flat.reshape(-1, channels).T


@pytest.mark.parametrize('channels', [1, 2, 3])
def test_riff_pcm_and_float_codings(tmp_path, channels):
    rng = np.random.default_rng(10 + channels)
    n = 1001 * channels
    cases = []
    u8 = rng.integers(0, 256, size=n, dtype=np.int64)
    cases.append((u8.astype(np.uint8).tobytes(), 1, 8, (u8 - 128).astype(np.float32) * np.float32(1 / 128)))
    s16 = _ints(rng, n, 16)
    cases.append((s16.astype('<i2').tobytes(), 1, 16, s16.astype(np.float32) * np.float32(1 / 32768)))
    s24 = _ints(rng, n, 24)
    cases.append((_i24_bytes(s24), 1, 24, s24.astype(np.float32) * np.float32(2.0 ** -23)))
    s32 = _ints(rng, n, 32)
    cases.append((s32.astype('<i4').tobytes(), 1, 32, s32.astype(np.float32) * np.float32(2.0 ** -31)))
    f32 = rng.standard_normal(n).astype(np.float32)
    cases.append((f32.astype('<f4').tobytes(), 3, 32, f32))
    f64 = rng.standard_normal(n)
    cases.append((f64.astype('<f8').tobytes(), 3, 64, f64.astype(np.float32)))
    for i, (payload, tag, bits, expect) in enumerate(cases):
        for ext in (False, True):
            p = str(tmp_path / ('c%d_%d.wav' % (i, ext)))
            _wav(p, payload, tag, channels, 22050 + i, bits, extensible=ext)
            y, sr = audio.read(p)
            assert sr == 22050 + i
            assert y.dtype == np.float32 and y.shape == ((n,) if channels == 1 else (channels, n // channels))
            assert np.array_equal(y, _frames(expect, channels)), (bits, tag, ext)
    # exactness of the 16/24-bit scalings: integers times a power of two
    assert np.array_equal(s24.astype(np.float32) * np.float32(2.0 ** -23), s24 / 2.0 ** 23)


def test_riff_chunk_walk(tmp_path):
    rng = np.random.default_rng(2)
    s = _ints(rng, 4001, 16)
    expect = s.astype(np.float32) / np.float32(32768)
    extra = [(b'LIST', b'INFOISFT' + struct.pack('<I', 5) + b'synth'), (b'odd ', b'abc'), (b'fact', struct.pack('<I', 4001))]
    p = str(tmp_path / 'chunks.wav')
    _wav(p, s.astype('<i2').tobytes(), 1, 1, 48000, 16, extra_chunks=extra)
    y, sr = audio.read(p)
    assert sr == 48000 and np.array_equal(y, expect)
    for size in (0, 0xFFFFFFFF):                       # streamed writers: data to the end of the file
        p = str(tmp_path / ('stream%d.wav' % size))
        _wav(p, s.astype('<i2').tobytes(), 1, 1, 44100, 16, extra_chunks=extra[:2], data_size=size)
        y, sr = audio.read(p)
        assert sr == 44100 and np.array_equal(y, expect)
    # a trailing odd byte (a partial frame) is dropped
    p = str(tmp_path / 'partial.wav')
    _wav(p, s.astype('<i2').tobytes() + b'\x07', 1, 1, 16000, 16)
    assert np.array_equal(audio.read(p)[0], expect)


@pytest.mark.parametrize('nbytes', [2, 3, 4])
@pytest.mark.parametrize('big', [False, True])
@pytest.mark.parametrize('channels', [1, 2])
def test_sphere(tmp_path, nbytes, big, channels):
    rng = np.random.default_rng(nbytes * 10 + big + 100 * channels)
    s = _ints(rng, 3000 * channels, 8 * nbytes)
    if nbytes == 2:
        payload = s.astype('>i2' if big else '<i2').tobytes()
    elif nbytes == 3:
        payload = _i24_bytes(s, big)
    else:
        payload = s.astype('>i4' if big else '<i4').tobytes()
    scale = {2: 1 / 32768, 3: 2.0 ** -23, 4: 2.0 ** -31}[nbytes]
    expect = _frames(s.astype(np.float32) * np.float32(scale), channels)
    p = str(tmp_path / 'x.wav')
    _sphere(p, payload, 16000 if nbytes == 2 else 8000, channels, nbytes, '10' if big else '01')
    y, sr = audio.read(p)
    assert sr == (16000 if nbytes == 2 else 8000) and np.array_equal(y, expect)
    # header size taken from line 2; sample_count bounds the samples read
    _sphere(p, payload, 16000, channels, nbytes, '10' if big else '01', header_size=2048, count=1000)
    y, _ = audio.read(p)
    assert np.array_equal(y, expect[..., :1000])


def test_timit_style_header(tmp_path):
    rng = np.random.default_rng(5)
    s = _ints(rng, 7000, 16)
    p = str(tmp_path / 'SA1.WAV')
    _sphere(p, s.astype('<i2').tobytes(), 16000, 1, 2, '01')
    with open(p, 'rb') as f:
        head = f.read(1024)
    assert head.startswith(b'NIST_1A\n   1024\n') and b'end_head' in head
    y, sr = audio.read(p)
    assert sr == 16000 and np.array_equal(y, s.astype(np.float32) / np.float32(32768))


def _read_wav_16k(path):
    """The previous loader (preprocess_all.read_wav before any-rate decoding), restated."""
    with wave.open(path, 'rb') as w:
        assert w.getframerate() == 16000 and w.getsampwidth() == 2
        data = np.frombuffer(w.readframes(w.getnframes()), dtype='<i2').astype(np.float32) / 32768.0
        if w.getnchannels() > 1:
            data = data.reshape(-1, w.getnchannels()).mean(1)
    return data


@pytest.mark.parametrize('channels', [1, 2])
def test_16k_pcm16_is_what_the_previous_loader_gave(tmp_path, channels):
    rng = np.random.default_rng(7 + channels)
    s = _ints(rng, 16000 * channels + channels, 16)
    p = str(tmp_path / 'a.wav')
    with wave.open(p, 'wb') as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(s.astype('<i2').tobytes())
    y, sr = audio.read(p)
    m = audio.to_mono(y)
    old = _read_wav_16k(p)
    assert sr == 16000 and m.dtype == np.float32 and np.array_equal(m, old)
    assert m.tobytes() == old.tobytes()
    # load keeps a 16-kHz file as it was decoded (no resampling, no copy to the GPU)
    y2, sr2 = audio.load(p)
    assert sr2 == 16000 and isinstance(y2, np.ndarray) and np.array_equal(y2, old)


def test_to_mono_sums_in_order():
    rng = np.random.default_rng(3)
    y = rng.standard_normal((3, 500)).astype(np.float32)
    expect = ((y[0] + y[1]) + y[2]) / np.float32(3)
    assert np.array_equal(audio.to_mono(y), expect)
    assert np.array_equal(audio.to_mono(y), y.T.reshape(-1, 3).mean(1))
    assert audio.to_mono(y[0]) is not None and np.array_equal(audio.to_mono(y[0]), y[0])


def test_unsupported_codings_raise_naming_them(tmp_path):
    p = str(tmp_path / 'shorten.wav')
    _sphere(p, b'\x00' * 64, 16000, 1, 2, '01', coding='pcm,embedded-shorten-v2.00')
    with pytest.raises(ValueError, match='shorten'):
        audio.read(p)
    p = str(tmp_path / 'ulaw.sph')
    _sphere(p, b'\x00' * 64, 8000, 1, 2, '01', coding='ulaw')
    with pytest.raises(ValueError, match='ulaw'):
        audio.read(p)
    p = str(tmp_path / 'one.sph')
    _sphere(p, b'\x00' * 64, 8000, 1, 1, '1')
    with pytest.raises(ValueError, match='sample_n_bytes 1'):
        audio.read(p)
    p = str(tmp_path / 'mulaw.wav')
    _wav(p, b'\x00' * 64, 7, 1, 8000, 8)
    with pytest.raises(ValueError, match='mu-law'):
        audio.read(p)
    p = str(tmp_path / 'alaw.wav')
    _wav(p, b'\x00' * 64, 6, 1, 8000, 8)
    with pytest.raises(ValueError, match='A-law'):
        audio.read(p)
    p = str(tmp_path / 'adpcm.wav')
    _wav(p, b'\x00' * 64, 0x11, 1, 8000, 4)
    with pytest.raises(ValueError, match='0x0011'):
        audio.read(p)
    p = str(tmp_path / 'junk.wav')
    open(p, 'wb').write(b'OggS' + b'\x00' * 60)
    with pytest.raises(ValueError, match='neither RIFF'):
        audio.read(p)
    with pytest.raises(ValueError, match='kaiser_best'):
        audio.load(p, res_type='kaiser_fast')

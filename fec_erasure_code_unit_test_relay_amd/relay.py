"""Relay symbol-wise decode-and-forward (SWDF) over the MI355X C ABI (include/fec_amd.h,
fec_swdf_*).

Mirrors what Decoder_Symbol_Wise (src/Decoder_Symbol_Wise.cpp) does at the relay
(``symbol_wise_encode_1`` after ``push_current_codeword`` / ``rotate_pointers_and_insert_zero_word``,
driven by Variable_Rate_FEC_Decoder::receive_message_and_symbol_wise_encode, :950-1601) and at the
destination (``symbol_wise_decode_1`` + ``extract_data``, :1603-1879), batched over many packets
of one relay stream held in HBM.
"""
from __future__ import annotations

import ctypes

from ._lib import FEC_ERR_ARG, FecError, check, lib


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class SymbolWiseRelay:
    """Fixed-rate SWDF chain: source (T1, N1, N1) -> relay -> destination with (T2, N2), where
    k = T1-N1+1 = T2-N2+1 (the relay keeps the data symbols and changes the code length)."""

    def __init__(self, max_payload: int, T1: int, N1: int, T2: int, N2: int):
        h = ctypes.c_void_p()
        check(lib().fec_swdf_create(max_payload, T1, N1, T2, N2, ctypes.byref(h)), "fec_swdf_create")
        self._h = h
        v = [ctypes.c_int() for _ in range(6)]
        check(lib().fec_swdf_geometry(h, *[ctypes.byref(x) for x in v]), "fec_swdf_geometry")
        self.k, self.n1, self.n2, self.S, self.frame_bytes, self.delay = (x.value for x in v)
        self.L = max_payload
        self._work = None

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                lib().fec_swdf_destroy(self._h)
            except Exception:
                pass
            self._h = None

    def relay(self, codewords, erasure, frames=None, flag=None):
        """symbol_wise_encode_1 for seqs 0..P-1: source codewords [P, >= S*n1] uint8 (zero-padded
        rows) and hop-1 erasure flags [P] -> (frames [P, frame_bytes], flags [P] uint8)."""
        import torch
        assert codewords.dtype == torch.uint8 and codewords.is_cuda and codewords.is_contiguous()
        assert codewords.dim() == 2 and codewords.shape[1] >= self.S * self.n1
        P = codewords.shape[0]
        assert erasure.dtype == torch.uint8 and erasure.is_cuda and erasure.is_contiguous() and erasure.numel() >= P
        if frames is None:
            frames = torch.empty((P, self.frame_bytes), dtype=torch.uint8, device=codewords.device)
        assert frames.shape == (P, self.frame_bytes) and frames.is_contiguous() and frames.dtype == torch.uint8
        if flag is None:
            flag = torch.empty(P, dtype=torch.uint8, device=codewords.device)
        assert flag.numel() >= P and flag.dtype == torch.uint8 and flag.is_contiguous()
        nbytes = int(lib().fec_swdf_workspace_bytes(self._h, P))
        if self._work is None or self._work.numel() < nbytes:
            self._work = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=codewords.device)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(lib().fec_swdf_relay_batch(self._h, _ptr(codewords), codewords.shape[1], _ptr(erasure), P,
                                         _ptr(frames), _ptr(flag), _ptr(self._work), self._work.numel(),
                                         stream), "fec_swdf_relay_batch")
        return frames, flag

    def destination(self, frames, erasure, out=None, flag=None):
        """symbol_wise_decode_1 + extract_data for seqs 0..P-1: relay frames [P, frame_bytes] and
        hop-2 erasure flags [P] -> (data_with_header rows [P, S*k] (row t = source packet
        t - delay), flags [P] uint8)."""
        import torch
        assert frames.dtype == torch.uint8 and frames.is_cuda and frames.is_contiguous()
        assert frames.dim() == 2 and frames.shape[1] == self.frame_bytes
        P = frames.shape[0]
        assert erasure.dtype == torch.uint8 and erasure.is_cuda and erasure.is_contiguous() and erasure.numel() >= P
        if out is None:
            out = torch.empty((P, self.S * self.k), dtype=torch.uint8, device=frames.device)
        assert out.shape == (P, self.S * self.k) and out.is_contiguous() and out.dtype == torch.uint8
        if flag is None:
            flag = torch.empty(P, dtype=torch.uint8, device=frames.device)
        assert flag.numel() >= P and flag.dtype == torch.uint8 and flag.is_contiguous()
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(lib().fec_swdf_destination_batch(self._h, _ptr(frames), _ptr(erasure), P, _ptr(out), _ptr(flag),
                                               stream), "fec_swdf_destination_batch")
        return out, flag


class RelayStreamGroup:
    """``nstreams`` independent SWDF chains of one (max_payload, T1, N1, T2, N2) (fec_relay_streams_*):
    one Decoder_Symbol_Wise per stream and side, its state on the device between calls.  Each call
    hands over the next packet, or the next ``counts[m]`` packets, of every listed stream in one
    launch; per stream the rows of all calls together are SymbolWiseRelay.relay / .destination over
    the stream's whole sequence.  A relay node uses ``relay``, a destination node ``destination``."""

    def __init__(self, max_payload: int, T1: int, N1: int, T2: int, N2: int, nstreams: int):
        h = ctypes.c_void_p()
        check(lib().fec_relay_streams_create(max_payload, T1, N1, T2, N2, nstreams, ctypes.byref(h)),
              "fec_relay_streams_create")
        self._h = h
        v = [ctypes.c_int() for _ in range(7)]
        check(lib().fec_relay_streams_geometry(h, *[ctypes.byref(x) for x in v]), "fec_relay_streams_geometry")
        self.k, self.n1, self.n2, self.S, self.cw_bytes, self.frame_bytes, self.delay = (x.value for x in v)
        self.out_bytes = self.S * self.k
        self.L, self.nstreams = max_payload, nstreams
        self.codes = [(T1, N1, T2, N2)]
        self.code_of = [0] * nstreams

    @classmethod
    def mixed(cls, max_payload: int, tuples, code_of) -> "RelayStreamGroup":
        """A group whose stream s runs code tuples[code_of[s]] = (T1, N1, T2, N2)
        (fec_relay_streams_create_mixed): one call serves streams of different codes in one launch per
        side.  Every row array has one stride for the group: ``cw_bytes`` (the least codeword row),
        ``frame_bytes`` and ``out_bytes`` are the largest of the codes'; a stream's codeword, frame or
        output row is the first geometry(s)[...] bytes of its row, and the rest of a frame or output
        row is zero.  k, n1, n2, S and delay are None: they are per stream."""
        import numpy as np
        if tuples is None or code_of is None:  # what the library answers to a null pointer
            raise FecError(FEC_ERR_ARG, "fec_relay_streams_create_mixed")
        tup = np.ascontiguousarray(tuples, dtype=np.int32).reshape(-1, 4)
        cof = np.ascontiguousarray(code_of, dtype=np.int32).reshape(-1)
        h = ctypes.c_void_p()
        check(lib().fec_relay_streams_create_mixed(max_payload, tup.ctypes.data_as(ctypes.c_void_p), tup.shape[0],
                                                   cof.ctypes.data_as(ctypes.c_void_p), cof.size, ctypes.byref(h)),
              "fec_relay_streams_create_mixed")
        self = cls.__new__(cls)
        self._h = h
        self.L, self.nstreams = max_payload, cof.size
        v = [ctypes.c_int() for _ in range(4)]
        check(lib().fec_relay_streams_codes(h, *[ctypes.byref(x) for x in v]), "fec_relay_streams_codes")
        nc, self.cw_bytes, self.frame_bytes, self.out_bytes = (x.value for x in v)
        assert nc == tup.shape[0]
        self.codes = [tuple(int(x) for x in t) for t in tup]
        self.code_of = [self.geometry(s)["code"] for s in range(cof.size)]
        if nc == 1:
            g = self.geometry(0)
            self.k, self.n1, self.n2, self.S, self.delay = (g[x] for x in ("k", "n1", "n2", "S", "delay"))
        else:
            self.k = self.n1 = self.n2 = self.S = self.delay = None
        return self

    def geometry(self, stream_id: int) -> dict:
        """Stream `stream_id`'s code index and that code's k, n1, n2, S, cw_bytes, frame_bytes,
        out_bytes and delay."""
        v = [ctypes.c_int() for _ in range(9)]
        check(lib().fec_relay_streams_stream_geometry(self._h, stream_id, *[ctypes.byref(x) for x in v]),
              "fec_relay_streams_stream_geometry")
        return dict(zip(("code", "k", "n1", "n2", "S", "cw_bytes", "frame_bytes", "out_bytes", "delay"),
                        (x.value for x in v)))

    def set_code(self, stream_id: int, code: int) -> None:
        """Stream `stream_id` becomes a fresh relay chain and a fresh destination chain of code `code`
        (seq counters 0, no erasure behind it); the old chain's remaining outputs are never produced."""
        check(lib().fec_relay_streams_set_code(self._h, stream_id, code), "fec_relay_streams_set_code")
        self.code_of[stream_id] = code

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                lib().fec_relay_streams_destroy(self._h)
            except Exception:
                pass
            self._h = None

    @staticmethod
    def _rows(ids, counts, erasure):
        """Host arrays of a call: ids int32 [M], counts int32 [M] or None (one packet of each), the
        R = sum(counts) flags.  A count < 1 is the library's to refuse; it adds no rows here."""
        import numpy as np
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        assert ids.ndim == 1
        if counts is None:
            R = ids.size
        else:
            counts = np.ascontiguousarray(counts, dtype=np.int32)
            assert counts.shape == ids.shape
            R = int(np.maximum(counts, 0).sum(dtype=np.int64))
        er = np.ascontiguousarray(erasure, dtype=np.uint8)
        assert er.size == R
        return ids, counts, er, R

    @staticmethod
    def _host(a):
        return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None

    def relay(self, ids, counts, erasure, codewords, frames=None, flag=None):
        """symbol_wise_encode_1 for the next counts[m] seqs of stream ids[m]: codewords [R, >=
        cw_bytes] uint8 on the GPU (rows as in StreamGroup.encode_burst: stream ids[m]'s from row
        sum(counts[:m]) on; any row stride, any alignment; rows of erased packets are never read),
        erasure R host flags -> (frames [R, frame_bytes], flags [R] uint8) on the GPU."""
        import torch
        ids, counts, er, R = self._rows(ids, counts, erasure)
        assert codewords.dtype == torch.uint8 and codewords.is_cuda and codewords.dim() == 2
        assert codewords.shape[0] == R and codewords.shape[1] >= self.cw_bytes
        assert R == 0 or codewords.stride(1) == 1
        if frames is None:
            frames = torch.empty((R, self.frame_bytes), dtype=torch.uint8, device=codewords.device)
        assert frames.shape == (R, self.frame_bytes) and frames.is_contiguous() and frames.dtype == torch.uint8
        if flag is None:
            flag = torch.empty(R, dtype=torch.uint8, device=codewords.device)
        assert flag.numel() >= R and flag.dtype == torch.uint8 and flag.is_contiguous()
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(lib().fec_relay_streams_relay(self._h, self._host(ids), self._host(counts), ids.size, self._host(er),
                                            _ptr(codewords), codewords.stride(0) if R else self.cw_bytes,
                                            _ptr(frames), _ptr(flag), stream), "fec_relay_streams_relay")
        return frames, flag

    def destination(self, ids, counts, erasure, frames, out=None, flag=None):
        """symbol_wise_decode_1 + extract_data for the next counts[m] seqs of stream ids[m]: frames
        [R, frame_bytes] on the GPU, erasure R host flags -> (data_with_header rows [R, out_bytes] (a row
        = source packet seq - delay of its stream), flags [R] uint8) on the GPU."""
        import torch
        ids, counts, er, R = self._rows(ids, counts, erasure)
        assert frames.dtype == torch.uint8 and frames.is_cuda and frames.is_contiguous()
        assert tuple(frames.shape) == (R, self.frame_bytes)
        if out is None:
            out = torch.empty((R, self.out_bytes), dtype=torch.uint8, device=frames.device)
        assert out.shape == (R, self.out_bytes) and out.is_contiguous() and out.dtype == torch.uint8
        if flag is None:
            flag = torch.empty(R, dtype=torch.uint8, device=frames.device)
        assert flag.numel() >= R and flag.dtype == torch.uint8 and flag.is_contiguous()
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(lib().fec_relay_streams_destination(self._h, self._host(ids), self._host(counts), ids.size,
                                                  self._host(er), _ptr(frames), _ptr(out), _ptr(flag), stream),
              "fec_relay_streams_destination")
        return out, flag

    def state(self, stream_id: int):
        """(seqs relayed, seqs delivered) of one stream."""
        a, b = ctypes.c_int64(), ctypes.c_int64()
        check(lib().fec_relay_streams_state(self._h, stream_id, ctypes.byref(a), ctypes.byref(b)),
              "fec_relay_streams_state")
        return a.value, b.value


def relay_streams_fit(relay: bool, max_payload: int, T1: int, N1: int, T2: int, N2: int):
    """Host only: whether one side of a relay stream group fits a CU's LDS -> (fits, packets per chunk
    of a long burst, that chunk's LDS bytes); FecError for a tuple the group refuses."""
    tp, lds = ctypes.c_int(), ctypes.c_int()
    st = lib().fec_relay_streams_fit(int(relay), max_payload, T1, N1, T2, N2, ctypes.byref(tp), ctypes.byref(lds))
    if st < 0:
        check(st, "fec_relay_streams_fit")
    return bool(st), tp.value, lds.value


def relay_streams_mixed_fit(max_payload: int, tuples):
    """Host only: per code of a mixed relay stream group (relay chunk, relay LDS bytes, destination
    chunk, destination LDS bytes) as int32 arrays [ncodes] (fec_relay_streams_mixed_fit); FecError if a
    tuple is refused or does not fit."""
    import numpy as np
    tup = np.ascontiguousarray(tuples, dtype=np.int32).reshape(-1, 4)
    nc = tup.shape[0]
    res = [np.zeros(max(nc, 1), dtype=np.int32) for _ in range(4)]
    check(lib().fec_relay_streams_mixed_fit(max_payload, tup.ctypes.data_as(ctypes.c_void_p), nc,
                                            *[r.ctypes.data_as(ctypes.c_void_p) for r in res]),
          "fec_relay_streams_mixed_fit")
    return tuple(r[:nc] for r in res)


def relay_streams_plan_host(k: int, n: int, erasure, counts):
    """Host only: the flag half of one side for one stream from seq 0 fed in bursts of ``counts`` ->
    (window mask per row [P] uint32, loss flag per row [P] uint8)."""
    import numpy as np
    e = np.ascontiguousarray(erasure, dtype=np.uint8)
    c = np.ascontiguousarray(counts, dtype=np.int32)
    assert int(np.maximum(c, 0).sum(dtype=np.int64)) == e.size
    mask = np.zeros(e.size, dtype=np.uint32)
    flag = np.zeros(e.size, dtype=np.uint8)
    check(lib().fec_relay_streams_plan_host(k, n, e.ctypes.data_as(ctypes.c_void_p), c.ctypes.data_as(ctypes.c_void_p),
                                            c.size, mask.ctypes.data_as(ctypes.c_void_p),
                                            flag.ctypes.data_as(ctypes.c_void_p)), "fec_relay_streams_plan_host")
    return mask, flag


class MessageWiseRelayGroup:
    """``nstreams`` independent message-wise (type-1) relays at fixed rate, all of one (max_payload,
    code1 = (T1, B1, N1), code2 = (T2, B2, N2)) (fec_mw_relay_streams_*): per flow an FEC_Decoder of
    code1 feeding an FEC_Encoder of code2, its state on the device between calls.  Each call hands
    over the next packet, or the next ``counts[m]`` packets, of every listed flow and decodes and
    re-encodes them in one launch; per flow the rows of all calls together are
    StreamGroup(code1).decode_burst over the flow's hop-1 sequence, the first T1 rows dropped, then
    StreamGroup(code2).encode_burst.  The destination is StreamGroup(max_payload, *code2).decode_burst.
    ``mixed`` makes a group whose flows each run their own pair of codes and may change it (``set_code``);
    ``codes`` lists the group's pairs and ``code_of`` every flow's pair index (one pair and zeros here).
    This is not the reference's adaptive message-wise session (relay headers, acknowledgements)."""

    def __init__(self, max_payload: int, code1, code2, nstreams: int):
        (T1, B1, N1), (T2, B2, N2) = code1, code2
        h = ctypes.c_void_p()
        check(lib().fec_mw_relay_streams_create(max_payload, T1, B1, N1, T2, B2, N2, nstreams, ctypes.byref(h)),
              "fec_mw_relay_streams_create")
        self._h = h
        v = [ctypes.c_int() for _ in range(3)]
        check(lib().fec_mw_relay_streams_geometry(h, *[ctypes.byref(x) for x in v]), "fec_mw_relay_streams_geometry")
        self.cw1_bytes, self.cw2_bytes, self.delay = (x.value for x in v)
        self.L, self.nstreams = max_payload, nstreams
        self.code1, self.code2 = (T1, B1, N1), (T2, B2, N2)
        self.codes = [(self.code1, self.code2)]
        self.code_of = [0] * nstreams

    @classmethod
    def mixed(cls, max_payload: int, pairs, code_of) -> "MessageWiseRelayGroup":
        """A group whose flow s runs pair pairs[code_of[s]] = ((T1, B1, N1), (T2, B2, N2)), or a row
        of an [ncodes, 6] array (fec_mw_relay_streams_create_mixed): one call serves flows of different
        pairs in one launch.  Every row array has one stride for the group: ``cw1_bytes`` (the least
        codeword row) and ``cw2_bytes`` are the largest of the pairs'; a flow's hop-1 codeword or hop-2
        codeword is the first geometry(s)[...] bytes of its row, and the rest of an output row is zero.
        delay, code1 and code2 are None when there are several pairs: they are per flow."""
        import numpy as np
        if pairs is None or code_of is None:  # what the library answers to a null pointer
            raise FecError(FEC_ERR_ARG, "fec_mw_relay_streams_create_mixed")
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 6)
        cof = np.ascontiguousarray(code_of, dtype=np.int32).reshape(-1)
        h = ctypes.c_void_p()
        check(lib().fec_mw_relay_streams_create_mixed(max_payload, pr.ctypes.data_as(ctypes.c_void_p), pr.shape[0],
                                                      cof.ctypes.data_as(ctypes.c_void_p), cof.size, ctypes.byref(h)),
              "fec_mw_relay_streams_create_mixed")
        self = cls.__new__(cls)
        self._h = h
        self.L, self.nstreams = max_payload, cof.size
        v = [ctypes.c_int() for _ in range(3)]
        check(lib().fec_mw_relay_streams_codes(h, *[ctypes.byref(x) for x in v]), "fec_mw_relay_streams_codes")
        nc, self.cw1_bytes, self.cw2_bytes = (x.value for x in v)
        assert nc == pr.shape[0]
        self.codes = [(tuple(int(x) for x in p[:3]), tuple(int(x) for x in p[3:])) for p in pr]
        self.code_of = [self.geometry(s)["code"] for s in range(cof.size)]
        if nc == 1:
            self.delay = self.geometry(0)["delay"]
            self.code1, self.code2 = self.codes[0]
        else:
            self.delay = self.code1 = self.code2 = None
        return self

    def geometry(self, stream_id: int) -> dict:
        """Flow `stream_id`'s pair index and that pair's k1, n1, k2, n2, cw1_bytes, cw2_bytes and delay."""
        v = [ctypes.c_int() for _ in range(8)]
        check(lib().fec_mw_relay_streams_stream_geometry(self._h, stream_id, *[ctypes.byref(x) for x in v]),
              "fec_mw_relay_streams_stream_geometry")
        return dict(zip(("code", "k1", "n1", "k2", "n2", "cw1_bytes", "cw2_bytes", "delay"), (x.value for x in v)))

    def set_code(self, stream_id: int, code: int) -> None:
        """Flow `stream_id` becomes a fresh hop-1 decoder and a fresh hop-2 encoder of pair `code` (seq 0,
        no erasure behind it); the old pair's last T1 messages are never forwarded."""
        check(lib().fec_mw_relay_streams_set_code(self._h, stream_id, code), "fec_mw_relay_streams_set_code")
        self.code_of[stream_id] = code

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                lib().fec_mw_relay_streams_destroy(self._h)
            except Exception:
                pass
            self._h = None

    def relay(self, ids, counts, erasure, codewords, out=None, out_len=None, fate=None):
        """The next counts[m] hop-1 seqs of flow ids[m] (counts None: one of each): codewords [R, >=
        cw1_bytes] uint8 on the GPU, untrimmed (flow ids[m]'s from row sum(counts[:m]) on; any row
        stride, any alignment; rows of erased packets are never read), erasure R host flags ->
        (hop-2 codewords [R, cw2_bytes] uint8, trimmed sizes [R] int32, fates [R] uint8: 0 none, 1
        copied, 2 recovered, 3 lost) on the GPU.  A row of hop-1 seq < delay is zero with size 0."""
        import torch
        ids, counts, er, R = RelayStreamGroup._rows(ids, counts, erasure)
        assert codewords.dtype == torch.uint8 and codewords.is_cuda and codewords.dim() == 2
        assert codewords.shape[0] == R and (R == 0 or codewords.stride(1) == 1)
        dev = codewords.device
        if out is None:
            out = torch.empty((R, self.cw2_bytes), dtype=torch.uint8, device=dev)
        assert tuple(out.shape) == (R, self.cw2_bytes) and out.is_contiguous() and out.dtype == torch.uint8
        if out_len is None:
            out_len = torch.empty(R, dtype=torch.int32, device=dev)
        assert out_len.numel() >= R and out_len.dtype == torch.int32 and out_len.is_contiguous()
        if fate is None:
            fate = torch.empty(R, dtype=torch.uint8, device=dev)
        assert fate.numel() >= R and fate.dtype == torch.uint8 and fate.is_contiguous()
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        h = RelayStreamGroup._host
        # the row stride goes to the library as it is: a stride below cw1_bytes is the library's to refuse
        check(lib().fec_mw_relay_streams_relay(self._h, h(ids), h(counts), ids.size, h(er), _ptr(codewords),
                                               codewords.stride(0) if R else self.cw1_bytes, _ptr(out),
                                               _ptr(out_len), _ptr(fate), stream), "fec_mw_relay_streams_relay")
        return out, out_len, fate

    def state(self, stream_id: int):
        """(hop-1 packets received, messages forwarded) of one flow."""
        a, b = ctypes.c_int64(), ctypes.c_int64()
        check(lib().fec_mw_relay_streams_state(self._h, stream_id, ctypes.byref(a), ctypes.byref(b)),
              "fec_mw_relay_streams_state")
        return a.value, b.value


def mw_relay_streams_fit(max_payload: int, code1, code2):
    """Host only: (packets per chunk of a burst cut in several, that chunk's LDS bytes) of a
    message-wise relay group of code1 = (T1, B1, N1) -> code2 = (T2, B2, N2); FecError for a pair the
    group refuses (a tuple StreamGroup refuses, or a smallest chunk that does not fit)."""
    tp, lds = ctypes.c_int(), ctypes.c_int()
    check(lib().fec_mw_relay_streams_fit(max_payload, *code1, *code2, ctypes.byref(tp), ctypes.byref(lds)),
          "fec_mw_relay_streams_fit")
    return tp.value, lds.value


def mw_relay_streams_mixed_fit(max_payload: int, pairs):
    """Host only: per pair of a mixed message-wise relay group (packets per chunk of a burst cut in
    several, that chunk's LDS bytes) as int32 arrays [ncodes] (fec_mw_relay_streams_mixed_fit); FecError
    if a pair is refused."""
    import numpy as np
    pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 6)
    nc = pr.shape[0]
    res = [np.zeros(max(nc, 1), dtype=np.int32) for _ in range(2)]
    check(lib().fec_mw_relay_streams_mixed_fit(max_payload, pr.ctypes.data_as(ctypes.c_void_p), nc,
                                               *[r.ctypes.data_as(ctypes.c_void_p) for r in res]),
          "fec_mw_relay_streams_mixed_fit")
    return tuple(r[:nc] for r in res)


class StateDependentRelay:
    """Fixed-rate SD-SWDF chain (RELAYING_TYPE 3): source (T1, N1, N1) -> relay
    (symbol_wise_encode_state_dependent, Decoder_Symbol_Wise.cpp:178-432) -> destination
    (symbol_wise_decode_state_dependent + extract_data, :487-546, :653-661), with
    k = T1-N1+1 = T2-N2+1 and T2 <= T1 <= T_TOT = 10.  The erasure flags of both hops are host
    arrays: they drive the host planner (the reference's per-packet control flow); the bytes stay
    on the GPU."""

    RECORD_HDR = 11

    def __init__(self, max_payload: int, T1: int, N1: int, T2: int, N2: int, sdbo: int = 0):
        h = ctypes.c_void_p()
        check(lib().fec_sdswdf_create(max_payload, T1, N1, T2, N2, sdbo, ctypes.byref(h)), "fec_sdswdf_create")
        self._h = h
        v = [ctypes.c_int() for _ in range(7)]
        check(lib().fec_sdswdf_geometry(h, *[ctypes.byref(x) for x in v]), "fec_sdswdf_geometry")
        self.k, self.n1, self.n2, self.S, self.blocks, self.frame_bytes, self.delay = (x.value for x in v)
        self.L = max_payload

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                lib().fec_sdswdf_destroy(self._h)
            except Exception:
                pass
            self._h = None

    @staticmethod
    def _host_flags(erasure, P):
        import numpy as np
        e = np.ascontiguousarray(np.asarray(erasure)[:P], dtype=np.uint8)
        assert e.size == P
        return e

    def relay(self, codewords, erasure, frames=None):
        """seqs 0..P-1: source codewords [P, >= S*n1] uint8 on the GPU (zero-padded rows; erased
        rows are never read), hop-1 flags [P] (host array) -> frames [P, frame_bytes]."""
        import torch
        assert codewords.dtype == torch.uint8 and codewords.is_cuda and codewords.is_contiguous()
        assert codewords.dim() == 2 and codewords.shape[1] >= self.S * self.n1
        P = codewords.shape[0]
        e = self._host_flags(erasure, P)
        if frames is None:
            frames = torch.empty((P, self.frame_bytes), dtype=torch.uint8, device=codewords.device)
        assert frames.shape == (P, self.frame_bytes) and frames.is_contiguous() and frames.dtype == torch.uint8
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(lib().fec_sdswdf_relay_batch(self._h, _ptr(codewords), codewords.shape[1],
                                           e.ctypes.data_as(ctypes.c_void_p), P, _ptr(frames), stream),
              "fec_sdswdf_relay_batch")
        return frames

    def destination(self, frames, erasure, out=None):
        """seqs 0..P-1: relay frames [P, frame_bytes] on the GPU, hop-2 flags [P] (host array) ->
        (data_with_header rows [P, S*k] on the GPU (row t = source packet t - delay), flags [P]
        numpy uint8)."""
        import numpy as np
        import torch
        assert frames.dtype == torch.uint8 and frames.is_cuda and frames.is_contiguous()
        assert frames.dim() == 2 and frames.shape[1] == self.frame_bytes
        P = frames.shape[0]
        e = self._host_flags(erasure, P)
        if out is None:
            out = torch.empty((P, self.S * self.k), dtype=torch.uint8, device=frames.device)
        assert out.shape == (P, self.S * self.k) and out.is_contiguous() and out.dtype == torch.uint8
        flag = np.zeros(P, dtype=np.uint8)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(lib().fec_sdswdf_destination_batch(self._h, _ptr(frames), e.ctypes.data_as(ctypes.c_void_p), P,
                                                 _ptr(out), flag.ctypes.data_as(ctypes.c_void_p), stream),
              "fec_sdswdf_destination_batch")
        return out, flag

    def relay_plan(self, erasure):
        """The relay's host plan alone (no GPU): (record id per seq [P] int32, records [R, 11 +
        n2*n1] uint8: header bytes, then n2 rows of n1 coefficients)."""
        import numpy as np
        e = self._host_flags(erasure, len(erasure))
        P = e.size
        ids = np.zeros(P, dtype=np.int32)
        n = ctypes.c_int64()
        rb = ctypes.c_int()
        check(lib().fec_sdswdf_relay_plan(self._h, e.ctypes.data_as(ctypes.c_void_p), P,
                                          ids.ctypes.data_as(ctypes.c_void_p), None, 0, ctypes.byref(n),
                                          ctypes.byref(rb)), "fec_sdswdf_relay_plan")
        rec = np.zeros((n.value, rb.value), dtype=np.uint8)
        check(lib().fec_sdswdf_relay_plan(self._h, e.ctypes.data_as(ctypes.c_void_p), P,
                                          ids.ctypes.data_as(ctypes.c_void_p), rec.ctypes.data_as(ctypes.c_void_p),
                                          rec.size, ctypes.byref(n), ctypes.byref(rb)), "fec_sdswdf_relay_plan")
        return ids, rec

    def dest_plan(self, erasure, headers):
        """The destination's host plan alone (no GPU): headers [P, 11] = bytes 2..12 of every
        frame -> (record id per seq, records [R, k*n2], flags [P])."""
        import numpy as np
        e = self._host_flags(erasure, len(erasure))
        P = e.size
        hd = np.ascontiguousarray(headers[:P], dtype=np.uint8)
        assert hd.shape == (P, 11)
        ids = np.zeros(P, dtype=np.int32)
        fl = np.zeros(P, dtype=np.uint8)
        n = ctypes.c_int64()
        rb = ctypes.c_int()
        args = [self._h, e.ctypes.data_as(ctypes.c_void_p), hd.ctypes.data_as(ctypes.c_void_p), P,
                ids.ctypes.data_as(ctypes.c_void_p), fl.ctypes.data_as(ctypes.c_void_p)]
        check(lib().fec_sdswdf_dest_plan(*args, None, 0, ctypes.byref(n), ctypes.byref(rb)), "fec_sdswdf_dest_plan")
        rec = np.zeros((n.value, rb.value), dtype=np.uint8)
        check(lib().fec_sdswdf_dest_plan(*args, rec.ctypes.data_as(ctypes.c_void_p), rec.size, ctypes.byref(n),
                                         ctypes.byref(rb)), "fec_sdswdf_dest_plan")
        return ids, rec, fl


T_TOT = 10  # FEC_Macro.h


class AdaptiveRelay:
    """The relay chain under variable rate (RELAYING_TYPE 2 or 3 through code switches,
    Variable_Rate_FEC_Decoder.cpp:600-740 relay, :1423-1600 / :1772-1873 destination), batched:
    ``schedule`` = [(seq, T, N), ...] source codes (T, N, N), the first at seq 0, each at least
    T_TOT + 1 after the previous (the T_TOT + 1 double-coded seqs of a switch); hop 2 re-encodes
    with the same (T, N).  ``run`` returns what the relay sends per seq ([BE16 size][new part]
    [old part during double coding]) and what the reporting destination object outputs per seq
    (fec_relay_vr_* in include/fec_amd.h)."""

    def __init__(self, relay_type: int, max_payload: int, schedule, P: int):
        import numpy as np
        sched = np.ascontiguousarray(np.asarray(schedule, dtype=np.int32).reshape(-1, 3))
        h = ctypes.c_void_p()
        check(lib().fec_relay_vr_create(relay_type, max_payload, sched.ctypes.data_as(ctypes.c_void_p), sched.shape[0],
                                        P, ctypes.byref(h)), "fec_relay_vr_create")
        self._h = h
        v = [ctypes.c_int() for _ in range(3)]
        check(lib().fec_relay_vr_geometry(h, *[ctypes.byref(x) for x in v]), "fec_relay_vr_geometry")
        self.frame_stride, self.out_stride, self.codes = (x.value for x in v)
        self.type, self.L, self.P = relay_type, max_payload, P

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                lib().fec_relay_vr_destroy(self._h)
            except Exception:
                pass
            self._h = None

    @staticmethod
    def schedule_from_plan(plan, P: int):
        """Switch points of a variable-rate plan's encoder instances (fec_vr.VrPlan.encoders:
        (T, B, N, first, role switch, end), adaptive tuples B = N) that start at least T_TOT + 1
        seqs after the previous kept one, as the relay's code schedule."""
        sched = []
        for T, B, N, first, _sw, _end in plan.encoders.tolist():
            if first >= P:
                break
            if not sched or first >= sched[-1][0] + T_TOT + 1:
                sched.append((int(first), int(T), int(N)))
        return sched

    def run(self, payload, e1, e2):
        """payload [P, L] uint8 on the GPU (source packet t), hop erasure flags e1 / e2 (P host
        bytes, numpy) -> (frames [P, frame_stride], frame_len [P] int32, out [P, out_stride], flags
        [P] numpy uint8)."""
        import numpy as np
        import torch
        assert payload.dtype == torch.uint8 and payload.is_cuda and payload.is_contiguous()
        assert tuple(payload.shape) == (self.P, self.L)
        e1 = np.ascontiguousarray(np.asarray(e1, dtype=np.uint8)[:self.P])
        e2 = np.ascontiguousarray(np.asarray(e2, dtype=np.uint8)[:self.P])
        assert e1.size == self.P and e2.size == self.P
        dev = payload.device
        frames = torch.empty((self.P, self.frame_stride), dtype=torch.uint8, device=dev)
        flen = torch.empty(self.P, dtype=torch.int32, device=dev)
        out = torch.empty((self.P, self.out_stride), dtype=torch.uint8, device=dev)
        flags = np.zeros(self.P, dtype=np.uint8)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(lib().fec_relay_vr_run(self._h, _ptr(payload), e1.ctypes.data_as(ctypes.c_void_p),
                                     e2.ctypes.data_as(ctypes.c_void_p), _ptr(frames), _ptr(flen), _ptr(out),
                                     flags.ctypes.data_as(ctypes.c_void_p), stream), "fec_relay_vr_run")
        return frames, flen, out, flags


class RelaySession:
    """The two-hop adaptive relay session (RELAYING_TYPE 2 / 3 with N_INITIAL = N_INITIAL_2 = -1,
    application_local_simulation.cpp:71-593): source (Application_Layer_Sender with the relay's
    12-byte feedback, the relay-mode Variable_Rate_FEC_Encoder) -> hop 1 -> relay
    (receive_message_and_symbol_wise_encode + send_sym_wise_message) -> hop 2 -> destination
    (receive_message_and_symbol_wise_decode), for Q seqs over the hop patterns e1 / e2
    (fec_relay_session_* in include/fec_amd.h).  The control plane runs at construction (host, on
    the patterns alone); run() does the session's byte work on the GPU."""

    DW = 320  # destination output row

    def __init__(self, relay_type: int, Q: int, e1, e2, max_payload: int = 300):
        import numpy as np
        a = np.ascontiguousarray(np.asarray(e1, dtype=np.uint8))
        b = np.ascontiguousarray(np.asarray(e2, dtype=np.uint8))
        h = ctypes.c_void_p()
        check(lib().fec_relay_session_create(relay_type, max_payload, Q, a.ctypes.data_as(ctypes.c_void_p), a.size,
                                             b.ctypes.data_as(ctypes.c_void_p), b.size, ctypes.byref(h)),
              "fec_relay_session_create")
        self._h = h
        self.type, self.Q, self.L = relay_type, Q, max_payload
        st = np.zeros(16, np.int64)
        rt = np.zeros(4, np.float64)
        check(lib().fec_relay_session_info(h, st.ctypes.data_as(ctypes.c_void_p), rt.ctypes.data_as(ctypes.c_void_p)),
              "fec_relay_session_info")
        keys = ("Q", "relay_bytes", "src_switches", "relay_switches", "dest_switches", "dest_flags", "relay_calls",
                "lineages", "dest_outputs", "processed", "symbol_bytes", "encoder_instances", "longest_lineage",
                "relay_flags", "rate1_n", "rate2_n")
        self.stats = {k: int(v) for k, v in zip(keys, st)}
        self.stats.update(rate1=float(rt[0]), rate2=float(rt[1]), min_rate=float(rt[2]), control_ms=float(rt[3]))
        self.relay_off = np.zeros(Q + 1, np.int64)
        check(lib().fec_relay_session_relay_offsets(h, self.relay_off.ctypes.data_as(ctypes.c_void_p)),
              "fec_relay_session_relay_offsets")
        self.hop1_hdr = np.zeros((Q, 16), np.uint8)
        check(lib().fec_relay_session_hop1_headers(h, self.hop1_hdr.ctypes.data_as(ctypes.c_void_p)),
              "fec_relay_session_hop1_headers")
        self.proc = np.zeros(Q, np.uint8)
        self.flag = np.zeros(Q, np.uint8)
        check(lib().fec_relay_session_dest_meta(h, self.proc.ctypes.data_as(ctypes.c_void_p),
                                                self.flag.ctypes.data_as(ctypes.c_void_p)), "fec_relay_session_dest_meta")

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                lib().fec_relay_session_destroy(self._h)
            except Exception:
                pass
            self._h = None

    def run(self, payload, relay=None, out=None, lost=None, count=None):
        """payload [Q, L] uint8 on the GPU -> (relay packets [relay_bytes] (packet t at
        relay_off[t]..relay_off[t+1]), destination outputs [Q, 320], lost flags [Q], lost count [1])."""
        import torch
        assert payload.dtype == torch.uint8 and payload.is_cuda and payload.is_contiguous()
        assert tuple(payload.shape) == (self.Q, self.L)
        dev = payload.device
        if relay is None:
            relay = torch.empty(int(self.relay_off[-1]), dtype=torch.uint8, device=dev)
        if out is None:
            out = torch.empty((self.Q, self.DW), dtype=torch.uint8, device=dev)
        if lost is None:
            lost = torch.empty(self.Q, dtype=torch.uint8, device=dev)
        if count is None:
            count = torch.empty(1, dtype=torch.int64, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(lib().fec_relay_session_run(self._h, _ptr(payload), _ptr(relay), _ptr(out), _ptr(lost), _ptr(count),
                                          stream), "fec_relay_session_run")
        return relay, out, lost, count

    def hop1_packets(self, stride: int):
        """After run(): the source's wire packets [Q, stride] (16-byte header + VR frame, zero padded)
        and their sizes [Q]."""
        import torch
        pk = torch.empty((self.Q, stride), dtype=torch.uint8, device="cuda")
        ln = torch.empty(self.Q, dtype=torch.int32, device="cuda")
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(lib().fec_relay_session_hop1(self._h, _ptr(pk), stride, _ptr(ln), stream), "fec_relay_session_hop1")
        return pk, ln


def relay_digest(frames, frame_len, out, flags, block: int = 100):
    """Per block of ``block`` seqs the CRC-32 of every seq's [frame_len LE32][frame][out][flag]
    (as tests/cpp/relay_dropin_test.cpp --digest writes for the reference-structured driver)."""
    import zlib
    import numpy as np
    fr = frames.cpu().numpy()
    fl = frame_len.cpu().numpy().astype(np.int64)
    ou = out.cpu().numpy()
    P = fr.shape[0]
    res = []
    for b0 in range(0, P, block):
        c = 0
        for t in range(b0, min(P, b0 + block)):
            c = zlib.crc32(int(fl[t]).to_bytes(4, "little"), c)
            c = zlib.crc32(fr[t, :fl[t]].tobytes(), c)
            c = zlib.crc32(ou[t].tobytes(), c)
            c = zlib.crc32(bytes([int(flags[t])]), c)
        res.append(c)
    return res

"""btsha1 -- ctypes binding of libbtsha1.so (the C-ABI in include/bt_sha1.h).

This is the binding a Python caller (tests, bench.py) uses; C callers link the
library directly.  Device buffers are passed as raw integer
addresses (e.g. ``tensor.data_ptr()``) and streams as raw ``hipStream_t``
handles (``torch.cuda.current_stream().cuda_stream``), so nothing here depends
on torch.  There is no fallback: if the library cannot be loaded, importing
this module raises, and every call that fails on the GPU raises BtSha1Error
with the library's own message.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BT_SHA1_LIB", os.path.join(HERE, "libbtsha1.so"))
CHUNK = 512 * 1024  # BT_CHUNK_SIZE, chunk.h:16
DIGEST = 20  # SHA1_HASH_SIZE, sha.h:34


class BtSha1Error(RuntimeError):
    pass


if not os.path.exists(LIB_PATH):
    raise ImportError(f"libbtsha1.so not built at {LIB_PATH}: run `make` (or __graft_entry__.build())")
lib = ctypes.CDLL(LIB_PATH)

_u8p = ctypes.POINTER(ctypes.c_uint8)
_vp = ctypes.c_void_p
_u64 = ctypes.c_uint64
_i64 = ctypes.c_int64


class Verdict(ctypes.Structure):
    _fields_ = [("tag", ctypes.c_uint64), ("ok", ctypes.c_int32), ("digest", ctypes.c_uint8 * 20)]


class SHA1Context(ctypes.Structure):  # include/sha.h (reference sha.h:39-50 layout)
    _fields_ = [("totalLength", ctypes.c_uint64), ("hash", ctypes.c_uint32 * 5),
                ("bufferLength", ctypes.c_uint32), ("buffer", ctypes.c_uint8 * 64)]


STATS_NODES = 8  # BT_SHA1_STATS_NODES


class PipelineStats(ctypes.Structure):  # include/bt_sha1.h bt_sha1_pipeline_stats
    _fields_ = [("chunks", ctypes.c_uint64), ("bytes", ctypes.c_uint64), ("batch_bytes", ctypes.c_uint64),
                ("batches", ctypes.c_uint32), ("staged", ctypes.c_int32), ("device", ctypes.c_int32),
                ("copy_threads", ctypes.c_int32), ("numa_nodes", ctypes.c_int32),
                ("gpu_numa_node", ctypes.c_int32), ("numa_policy", ctypes.c_int32),
                ("registered_batches", ctypes.c_int32), ("column_chunks", ctypes.c_uint32),
                ("total_s", ctypes.c_double), ("alloc_s", ctypes.c_double), ("fill_s", ctypes.c_double),
                ("wait_s", ctypes.c_double), ("register_s", ctypes.c_double), ("unregister_s", ctypes.c_double),
                ("lane_pages", ctypes.c_int32 * STATS_NODES), ("src_pages", ctypes.c_int32 * STATS_NODES),
                ("copy_pieces", ctypes.c_int32 * STATS_NODES)]


def _sig(name, res, *args):
    f = getattr(lib, name)
    f.restype = res
    f.argtypes = list(args)
    return f


_sig("bt_sha1_device_count", ctypes.c_int)
_sig("bt_sha1_set_device", ctypes.c_int, ctypes.c_int)
_sig("bt_sha1_last_error", ctypes.c_char_p)
_sig("bt_sha1_build_info", ctypes.c_char_p)
_sig("bt_sha1_set_ring_depth", ctypes.c_int, ctypes.c_int)
_sig("bt_sha1_set_variant", ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int)
_sig("bt_sha1_set_latency_batch", _u64, _u64)
_sig("bt_sha1_set_seglist_latency_batch", _u64, _u64)
_sig("bt_sha1_seglist_kernel_name", ctypes.c_char_p, _u64)
_sig("bt_sha1_chunks_dev", ctypes.c_int, _vp, _u64, _u64, _u64, _vp, _vp)
_sig("bt_sha1_verify_dev", ctypes.c_int, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp)
_sig("bt_sha1_column_dev", ctypes.c_int, _vp, _u64, _u64, _u64, ctypes.c_int, _vp, _u64, _vp, _vp, _vp, _vp)
_sig("bt_sha1_ragged_dev", ctypes.c_int, _vp, _vp, _vp, _u64, _vp, _vp)
_sig("bt_sha1_ragged_verify_dev", ctypes.c_int, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp)
_sig("bt_sha1_fill_synthetic", ctypes.c_int, _vp, _u64, _u64, _u64, _vp)
_sig("bt_sha1_chunks_host", _i64, _vp, _u64, _u64, _vp)
_sig("bt_sha1_host_register", ctypes.c_int, _vp, _u64)
_sig("bt_sha1_host_unregister", ctypes.c_int, _vp)
_sig("bt_sha1_chunks_host_multi", _i64, _vp, _u64, _u64, _vp, ctypes.c_int)
_sig("bt_sha1_chunks_host_devices", _i64, _vp, _u64, _u64, _vp, ctypes.POINTER(ctypes.c_int), ctypes.c_int)
_sig("bt_sha1_source_id", ctypes.c_char_p)
_sig("bt_sha1_set_chain_batch", _u64, _u64)
_sig("bt_sha1_kernel_name", ctypes.c_char_p, _u64)
_sig("bt_sha1_clock_probe", ctypes.c_int, _vp, _u64, _u64, _u64, _vp, _vp, _vp)
_sig("bt_sha1_wallclock_khz", _i64)
_sig("bt_sha1_debug_barrier_stats", ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int)
_sig("bt_sha1_debug_dropin_residue", _i64, ctypes.c_int)
_sig("bt_sha1_chunks_file", _i64, _vp, _u64, _vp, _u64)
_sig("bt_sha1_get_pipeline_stats", ctypes.c_int, ctypes.POINTER(PipelineStats))
_sig("bt_sha1_set_pageable_feed", ctypes.c_int, ctypes.c_int)
_sig("bt_sha1_verifier_create", _vp, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32)
_sig("bt_sha1_verifier_destroy", None, _vp)
_sig("bt_sha1_verifier_slot", _vp, _vp)
_sig("bt_sha1_verifier_commit", ctypes.c_int, _vp, _vp, ctypes.c_uint32, _vp, _u64)
_sig("bt_sha1_verifier_release", ctypes.c_int, _vp, _vp)
_sig("bt_sha1_verifier_submit", ctypes.c_int, _vp, _vp, ctypes.c_uint32, _vp, _u64)
_sig("bt_sha1_verifier_flush", ctypes.c_int, _vp)
_sig("bt_sha1_verifier_poll", ctypes.c_int, _vp, ctypes.POINTER(Verdict), ctypes.c_int)
_sig("bt_sha1_verifier_drain", ctypes.c_int, _vp, ctypes.POINTER(Verdict), ctypes.c_int)
_sig("bt_sha1_verifier_pending", _i64, _vp)


class VerifierStats(ctypes.Structure):  # include/bt_sha1.h bt_sha1_verifier_stats
    _fields_ = [(f, ctypes.c_uint64) for f in ("batches", "ragged_batches", "chunks", "short_chunks", "released")]


_sig("bt_sha1_verifier_create_ragged", _vp, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32)
_sig("bt_sha1_verifier_get_stats", ctypes.c_int, _vp, ctypes.POINTER(VerifierStats))


class Seg(ctypes.Structure):  # include/bt_sha1.h bt_sha1_seg
    _fields_ = [("off", ctypes.c_uint64), ("len", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class VerifierGatherStats(ctypes.Structure):  # include/bt_sha1.h bt_sha1_verifier_gather_stats
    _fields_ = [(f, ctypes.c_uint64) for f in ("gather_batches", "gather_chunks", "segments", "payload_bytes",
                                               "copied_bytes")]


_sig("bt_sha1_gather_dev", ctypes.c_int, _vp, _vp, _vp, _vp, _u64, _vp, _vp)
_sig("bt_sha1_gather_verify_dev", ctypes.c_int, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp)
_sig("bt_sha1_set_segchain_batch", _u64, _u64)


class PktGeom(ctypes.Structure):  # include/bt_sha1.h bt_sha1_pkt_geom
    _fields_ = [(f, ctypes.c_uint32) for f in ("stride", "header", "payload", "slot_pkts")]


_sig("bt_sha1_pkts_dev", ctypes.c_int, _vp, ctypes.POINTER(PktGeom), _vp, _vp, _vp, _vp, _u64, _vp, _vp)
_sig("bt_sha1_pkts_verify_dev", ctypes.c_int, _vp, ctypes.POINTER(PktGeom), _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp,
     _vp)
_sig("bt_sha1_segchain_dev", ctypes.c_int, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, ctypes.c_uint32, _vp)
_sig("bt_sha1_verifier_create_gather", _vp, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
     ctypes.c_uint32)
_sig("bt_sha1_verifier_commit_gather", ctypes.c_int, _vp, _vp, ctypes.POINTER(Seg), ctypes.c_uint32, _vp, _u64)
_sig("bt_sha1_verifier_get_gather_stats", ctypes.c_int, _vp, ctypes.POINTER(VerifierGatherStats))
_sig("bt_sha1_lookup_dev", ctypes.c_int, _vp, _u64, _vp, _u64, _vp, _vp)
_sig("bt_sha1_states_init_dev", ctypes.c_int, _vp, _u64, _vp)
_sig("bt_sha1_resume_dev", ctypes.c_int, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp)


class ReceiverStats(ctypes.Structure):  # include/bt_sha1.h bt_sha1_receiver_stats
    _fields_ = [("launches", ctypes.c_uint64), ("advance_launches", ctypes.c_uint64),
                ("advanced_bytes", ctypes.c_uint64), ("committed", ctypes.c_uint64), ("released", ctypes.c_uint64)]


_sig("bt_sha1_receiver_create", _vp, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32)
_sig("bt_sha1_receiver_destroy", None, _vp)
_sig("bt_sha1_receiver_slot", _vp, _vp)
_sig("bt_sha1_receiver_advance", ctypes.c_int, _vp, _vp, ctypes.c_uint32)
_sig("bt_sha1_receiver_commit", ctypes.c_int, _vp, _vp, ctypes.c_uint32, _vp, _u64)
_sig("bt_sha1_receiver_release", ctypes.c_int, _vp, _vp)
_sig("bt_sha1_receiver_poll", ctypes.c_int, _vp, ctypes.POINTER(Verdict), ctypes.c_int)
_sig("bt_sha1_receiver_drain", ctypes.c_int, _vp, ctypes.POINTER(Verdict), ctypes.c_int)
_sig("bt_sha1_receiver_pending", _i64, _vp)
_sig("bt_sha1_receiver_get_stats", ctypes.c_int, _vp, ctypes.POINTER(ReceiverStats))


class IntakeStats(ctypes.Structure):  # include/bt_sha1.h bt_sha1_intake_stats
    _fields_ = [(f, ctypes.c_uint64) for f in ("kicks", "launches", "entries", "max_entries", "advanced_bytes",
                                               "committed", "released", "deferred")]


_sig("bt_sha1_intake_create", _vp, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32)
_sig("bt_sha1_intake_destroy", None, _vp)
_sig("bt_sha1_intake_slot", _vp, _vp)
_sig("bt_sha1_intake_advance", ctypes.c_int, _vp, _vp, ctypes.c_uint32)
_sig("bt_sha1_intake_commit", ctypes.c_int, _vp, _vp, ctypes.c_uint32, _vp, _u64)
_sig("bt_sha1_intake_release", ctypes.c_int, _vp, _vp)
_sig("bt_sha1_intake_kick", ctypes.c_int, _vp)
_sig("bt_sha1_intake_sync", ctypes.c_int, _vp)
_sig("bt_sha1_intake_poll", ctypes.c_int, _vp, ctypes.POINTER(Verdict), ctypes.c_int)
_sig("bt_sha1_intake_drain", ctypes.c_int, _vp, ctypes.POINTER(Verdict), ctypes.c_int)
_sig("bt_sha1_intake_pending", _i64, _vp)
_sig("bt_sha1_intake_get_stats", ctypes.c_int, _vp, ctypes.POINTER(IntakeStats))
# bt_sha1_gather_resume_dev / bt_sha1_intake_create_gather / _append / _commit_gather under their exported names
_sig("bt_sha1_dgram_chain_dev", ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp)
_sig("bt_sha1_dgram_slots_create", _vp, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
     ctypes.c_uint32)
_sig("bt_sha1_dgram_slots_append", ctypes.c_int, _vp, _vp, _vp, ctypes.c_uint32)
_sig("bt_sha1_dgram_slots_commit", ctypes.c_int, _vp, _vp, _vp, _u64)


class ChunkEntry(ctypes.Structure):
    _fields_ = [("id", ctypes.c_int32), ("hash", ctypes.c_uint8 * 20)]


_sig("bt_chunks_parse_list", _i64, ctypes.c_char_p, ctypes.POINTER(ctypes.POINTER(ChunkEntry)))
_sig("bt_chunks_parse_master", _i64, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t,
     ctypes.POINTER(ctypes.POINTER(ChunkEntry)))
_sig("bt_chunks_free", None, ctypes.POINTER(ChunkEntry))
_sig("bt_chunks_write", ctypes.c_int, _vp, ctypes.c_char_p, _vp, ctypes.c_int64, ctypes.c_int32)
_sig("bt_hex2binary_checked", ctypes.c_int, ctypes.c_char_p, ctypes.c_int, _vp)
_sig("bt_chunks_last_error", ctypes.c_char_p)
_sig("SHA1Init", None, ctypes.POINTER(SHA1Context))
_sig("SHA1Update", None, ctypes.POINTER(SHA1Context), _vp, ctypes.c_uint32)
_sig("SHA1Final", None, ctypes.POINTER(SHA1Context), _vp)
_sig("shahash", None, _vp, ctypes.c_int, _vp)
_sig("binary2hex", None, _vp, ctypes.c_int, ctypes.c_char_p)
_sig("hex2binary", None, ctypes.c_char_p, ctypes.c_int, _vp)


def _check(rc, what):
    if rc is None or (isinstance(rc, int) and rc < 0):
        raise BtSha1Error(f"{what}: {lib.bt_sha1_last_error().decode()}")
    return rc


def last_error():
    return lib.bt_sha1_last_error().decode()


def device_count():
    return lib.bt_sha1_device_count()


def set_ring_depth(nbuf):
    _check(lib.bt_sha1_set_ring_depth(nbuf), "set_ring_depth")


def set_variant(nbuf, lines=1, nt=0):
    _check(lib.bt_sha1_set_variant(nbuf, lines, nt), "set_variant")


def set_latency_batch(max_chunks):
    """Batches of <= max_chunks take the latency kernel (0: never); returns the previous value."""
    return lib.bt_sha1_set_latency_batch(max_chunks)


def set_chain_batch(max_messages):
    """Ragged batches of <= max_messages take the chain kernel (0: never); returns the previous setting."""
    return lib.bt_sha1_set_chain_batch(max_messages)


def set_seglist_latency_batch(max_messages):
    """Segment-list batches of <= max_messages take k_sha1_gather_lat (0, the default: never;
    2**64 - 1: 128 per CU); returns the previous setting."""
    return lib.bt_sha1_set_seglist_latency_batch(max_messages)


def set_segchain_batch(max_messages):
    """Segment-list batches of <= max_messages take k_sha1_gather_chain, ahead of the latency
    form (0, the default: never; 2**64 - 1: 2 per CU); returns the previous setting."""
    return lib.bt_sha1_set_segchain_batch(max_messages)


def seglist_kernel_name(n):
    """Kernel a segment-list batch of n messages runs under the current setting and device."""
    return lib.bt_sha1_seglist_kernel_name(n).decode()


def build_info():
    return lib.bt_sha1_build_info().decode()


def source_id():
    """Id of the kernel sources compiled into the library (profiles record it)."""
    return lib.bt_sha1_source_id().decode()


def kernel_name(n_chunks):
    """Kernel a fixed-layout batch of n_chunks runs on the current device."""
    r = lib.bt_sha1_kernel_name(n_chunks)
    if r is None:
        raise BtSha1Error(f"bt_sha1_kernel_name: {last_error()}")
    return r.decode()


def clock_probe(d_in, n, chunk_len, pitch, d_digests, d_stamps, stream=None):
    """Stamped diagnostic build of the hot kernel (4 uint64 per wave into d_stamps)."""
    _check(lib.bt_sha1_clock_probe(d_in, n, chunk_len, pitch, d_digests, d_stamps, stream), "bt_sha1_clock_probe")


def wallclock_khz():
    return _check(lib.bt_sha1_wallclock_khz(), "bt_sha1_wallclock_khz")


def debug_barrier_stats(reset=False):
    """(waves checked, barriers executed, invariant misses) of the barrier-
    accounting build (make dbgbar, loaded with BT_SHA1_LIB); raises on the
    production library, which counts nothing."""
    out = (ctypes.c_uint64 * 3)()
    _check(lib.bt_sha1_debug_barrier_stats(out, 1 if reset else 0), "bt_sha1_debug_barrier_stats")
    return tuple(int(x) for x in out)


def debug_dropin_residue(device=0):
    """Nonzero bytes left in the drop-in calls' pinned staging on `device`
    (0 between calls: each shahash / SHA1Update / SHA1Final zeroes what it
    staged, as chunk.c:48 and sha.c:165-174 leave nothing behind)."""
    return _check(lib.bt_sha1_debug_dropin_residue(device), "bt_sha1_debug_dropin_residue")


# ---- device-resident (addresses are ints) ------------------------------------
def chunks_dev(d_in, n, chunk_len, pitch, d_digests, stream=None):
    _check(lib.bt_sha1_chunks_dev(d_in, n, chunk_len, pitch, d_digests, stream), "bt_sha1_chunks_dev")


def verify_dev(d_in, n, chunk_len, pitch, d_expected, d_ok, d_digests=None, stream=None):
    _check(lib.bt_sha1_verify_dev(d_in, n, chunk_len, pitch, d_expected, d_ok, d_digests, stream),
           "bt_sha1_verify_dev")


COLUMN_FIRST, COLUMN_MIDDLE, COLUMN_LAST = 0, 1, 2


def column_dev(d_col, n, pitch, width, part, d_state, msg_len=0, d_digests=None, d_expected=None, d_ok=None,
               stream=None):
    """One launch of the latency kernel's column form (diagnostic): `width`
    bytes of each of n chunks at d_col + i*pitch, chaining state in d_state
    (word k of chunk i at d_state[k*n + i]); COLUMN_LAST finishes a message of
    msg_len bytes into d_digests and / or the fused compare's d_ok."""
    _check(lib.bt_sha1_column_dev(d_col, n, pitch, width, part, d_state, msg_len, d_digests, d_expected, d_ok,
                                  stream), "bt_sha1_column_dev")


def ragged_dev(d_base, d_offsets, d_lens, n, d_digests, stream=None):
    _check(lib.bt_sha1_ragged_dev(d_base, d_offsets, d_lens, n, d_digests, stream), "bt_sha1_ragged_dev")


def ragged_verify_dev(d_base, d_offsets, d_lens, n, d_expected, d_ok, d_digests=None, stream=None):
    """ragged_dev with the fused compare: d_ok[i] = 1 iff SHA-1 of message i
    (d_lens[i] bytes, uint32, at d_base + d_offsets[i], uint64) equals
    d_expected[20*i ..].  Nothing needs any alignment; d_digests may be None."""
    _check(lib.bt_sha1_ragged_verify_dev(d_base, d_offsets, d_lens, n, d_expected, d_ok, d_digests, stream),
           "bt_sha1_ragged_verify_dev")


def gather_dev(d_base, d_segs, d_seg_first, d_seg_count, n, d_digests, stream=None):
    """Message i = the concatenation of the d_seg_count[i] (uint32) segments
    d_segs[d_seg_first[i] (uint64) ..], each a Seg: len bytes at d_base + off."""
    _check(lib.bt_sha1_gather_dev(d_base, d_segs, d_seg_first, d_seg_count, n, d_digests, stream),
           "bt_sha1_gather_dev")


def gather_verify_dev(d_base, d_segs, d_seg_first, d_seg_count, n, d_expected, d_ok, d_digests=None, stream=None):
    """gather_dev with the fused compare, as ragged_verify_dev."""
    _check(lib.bt_sha1_gather_verify_dev(d_base, d_segs, d_seg_first, d_seg_count, n, d_expected, d_ok, d_digests,
                                         stream), "bt_sha1_gather_verify_dev")


def pkts_dev(d_base, geom, d_slot_off, d_len, d_order, d_order_first, n, d_digests, stream=None):
    """Message i = d_len[i] (uint32) bytes held in the packet buffers of the
    slot at d_base + d_slot_off[i] (uint64, a multiple of 4): with geom a
    PktGeom, byte m lies in buffer d_order[d_order_first[i] + m // payload]
    (uint32 / uint64) at header + m % payload."""
    _check(lib.bt_sha1_pkts_dev(d_base, ctypes.byref(geom), d_slot_off, d_len, d_order, d_order_first, n, d_digests,
                                stream), "bt_sha1_pkts_dev")


def pkts_verify_dev(d_base, geom, d_slot_off, d_len, d_order, d_order_first, n, d_expected, d_ok, d_digests=None,
                    stream=None):
    """pkts_dev with the fused compare, as ragged_verify_dev."""
    _check(lib.bt_sha1_pkts_verify_dev(d_base, ctypes.byref(geom), d_slot_off, d_len, d_order, d_order_first, n,
                                       d_expected, d_ok, d_digests, stream), "bt_sha1_pkts_verify_dev")


def segchain_dev(d_base, d_segs, d_seg_first, d_seg_count, n, d_expected=None, d_ok=None, d_digests=None,
                 piece_bytes=0, stream=None):
    """One launch of k_sha1_gather_chain (diagnostic): gather_verify_dev's
    messages and results, one two-wave workgroup per message, whatever
    set_segchain_batch says.  d_expected and d_ok come together or not at all;
    piece_bytes (0: the production 2**31) caps the bytes of one pass."""
    _check(lib.bt_sha1_segchain_dev(d_base, d_segs, d_seg_first, d_seg_count, n, d_expected, d_ok, d_digests,
                                    piece_bytes, stream), "bt_sha1_segchain_dev")


def states_init_dev(d_states, n, stream=None):
    """d_states[5*i ..] = the SHA-1 IV for i < n: where resume_dev starts."""
    _check(lib.bt_sha1_states_init_dev(d_states, n, stream), "bt_sha1_states_init_dev")


def resume_dev(d_base, d_offsets, d_lens, d_totals, n, d_states, d_digests=None, d_expected=None, d_ok=None,
               stream=None):
    """One launch of the resumable chain kernel over n messages that are still
    arriving: message i's next d_lens[i] (uint32) bytes at d_base +
    d_offsets[i] (uint64), its chaining state at d_states[5*i ..].
    d_totals[i] (uint64) == 0 advances the state over the whole blocks;
    != 0 finishes a message of that many bytes into d_digests / d_ok."""
    _check(lib.bt_sha1_resume_dev(d_base, d_offsets, d_lens, d_totals, n, d_states, d_digests, d_expected, d_ok,
                                  stream), "bt_sha1_resume_dev")


def gather_resume_dev(d_base, d_segs, d_seg_pos, d_seg_first, d_seg_count, d_from, d_lens, d_totals, n, d_states,
                      d_digests=None, d_expected=None, d_ok=None, stream=None):
    """bt_sha1_gather_resume_dev: resume_dev over messages given as segment
    lists (gather_dev's tables, the segments listed so far) with d_seg_pos
    (uint64, parallel to d_segs: the message position of each segment's first
    byte).  Message bytes [d_from[i] (uint64, a 64-byte multiple), d_from[i] +
    d_lens[i] (uint32)) are hashed into d_states[5*i ..]; d_totals as resume_dev's."""
    _check(lib.bt_sha1_dgram_chain_dev(d_base, d_segs, d_seg_pos, d_seg_first, d_seg_count, d_from, d_lens, d_totals,
                                       n, d_states, d_digests, d_expected, d_ok, stream), "bt_sha1_gather_resume_dev")


def fill_synthetic(d_buf, nbytes, first_word, seed, stream=None):
    _check(lib.bt_sha1_fill_synthetic(d_buf, nbytes, first_word, seed, stream), "bt_sha1_fill_synthetic")


def lookup_dev(d_table, n_table, d_queries, n_queries, d_index, stream=None):
    _check(lib.bt_sha1_lookup_dev(d_table, n_table, d_queries, n_queries, d_index, stream), "bt_sha1_lookup_dev")


# ---- .chunks files (host-side parsing/formatting) ---------------------------------
def _entries(ptr, n):
    try:
        return [(ptr[i].id, bytes(ptr[i].hash)) for i in range(n)]
    finally:
        lib.bt_chunks_free(ptr)


def parse_chunk_list(path):
    """[(id, digest)] of a has/get .chunks file (util.c:64-111)."""
    p = ctypes.POINTER(ChunkEntry)()
    n = lib.bt_chunks_parse_list(str(path).encode(), ctypes.byref(p))
    if n < 0:
        raise BtSha1Error(lib.bt_chunks_last_error().decode())
    return _entries(p, n)


def parse_master(path):
    """(data file name, [(id, digest)]) of a master .chunks file (util.c:113-164)."""
    p = ctypes.POINTER(ChunkEntry)()
    name = ctypes.create_string_buffer(1024)
    n = lib.bt_chunks_parse_master(str(path).encode(), name, 1024, ctypes.byref(p))
    if n < 0:
        raise BtSha1Error(lib.bt_chunks_last_error().decode())
    return name.value.decode(), _entries(p, n)


def write_chunks(path, digests, master_name=None, first_id=0):
    libc = ctypes.CDLL(None)
    libc.fopen.restype = _vp
    libc.fopen.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    libc.fclose.argtypes = [_vp]
    raw = b"".join(digests)
    fp = libc.fopen(str(path).encode(), b"w")
    try:
        buf = (ctypes.c_uint8 * max(len(raw), 1)).from_buffer_copy(raw or b"\0")
        rc = lib.bt_chunks_write(fp, master_name.encode() if master_name else None, buf, len(digests), first_id)
    finally:
        libc.fclose(fp)
    if rc:
        raise BtSha1Error(lib.bt_chunks_last_error().decode())


def hex2binary_checked(h):
    hb = h.encode() if isinstance(h, str) else bytes(h)
    out = (ctypes.c_uint8 * max(len(hb) // 2, 1))()
    if lib.bt_hex2binary_checked(hb, len(hb), out):
        raise ValueError(f"not hex: {h!r}")
    return bytes(out)[:len(hb) // 2]


# ---- host ------------------------------------------------------------------------
def _host_buf(data):
    if isinstance(data, (bytes, bytearray)):
        b = (ctypes.c_uint8 * max(len(data), 1)).from_buffer_copy(bytes(data) or b"\0")
        return b, len(data)
    mv = memoryview(data).cast("B")
    arr = (ctypes.c_uint8 * max(mv.nbytes, 1)).from_buffer(mv) if not mv.readonly else \
        (ctypes.c_uint8 * max(mv.nbytes, 1)).from_buffer_copy(mv.tobytes() or b"\0")
    return arr, mv.nbytes


def _host_split(addr, nbytes, chunk_len, out, ndev, devs):
    if devs is not None:
        arr = (ctypes.c_int * max(len(devs), 1))(*devs)
        return _check(lib.bt_sha1_chunks_host_devices(addr, nbytes, chunk_len, out, arr, len(devs)),
                      "bt_sha1_chunks_host_devices")
    if ndev is not None:
        return _check(lib.bt_sha1_chunks_host_multi(addr, nbytes, chunk_len, out, ndev), "bt_sha1_chunks_host_multi")
    return _check(lib.bt_sha1_chunks_host(addr, nbytes, chunk_len, out), "bt_sha1_chunks_host")


def chunks_host(data, chunk_len=CHUNK, ndev=None, devs=None):
    """Digests of data cut into chunk_len pieces (short last piece): list of 20-byte values.
    ndev: split over the first ndev GPUs; devs: split over this list of device
    ids (repeats allowed: one worker per entry)."""
    buf, n = _host_buf(data)
    nch = (n + chunk_len - 1) // chunk_len
    out = (ctypes.c_uint8 * max(20 * nch, 1))()
    got = _host_split(buf, n, chunk_len, out, ndev, devs)
    raw = bytes(out)
    return [raw[20 * i:20 * i + 20] for i in range(got)]


def host_register(addr, nbytes):
    """Page-lock host memory at integer address `addr` (DMA without staging)."""
    _check(lib.bt_sha1_host_register(addr, nbytes), "bt_sha1_host_register")


def host_unregister(addr):
    _check(lib.bt_sha1_host_unregister(addr), "bt_sha1_host_unregister")


def chunks_host_addr(addr, nbytes, chunk_len=CHUNK, ndev=None, devs=None):
    """bt_sha1_chunks_host over raw host memory at `addr` (no copy on the Python side)."""
    nch = (nbytes + chunk_len - 1) // chunk_len
    out = (ctypes.c_uint8 * max(20 * nch, 1))()
    got = _host_split(addr, nbytes, chunk_len, out, ndev, devs)
    return bytes(out)[:20 * got]


PAGEABLE_FEEDS = {"register": 0, "stage": 1}


def set_pageable_feed(feed):
    """How bt_sha1_chunks_host feeds pageable input >= 64 MiB: "register" (page-lock
    batch by batch, DMA in place; the default) or "stage" (copy into the staging
    lanes).  Returns the previous setting's name."""
    prev = _check(lib.bt_sha1_set_pageable_feed(PAGEABLE_FEEDS[feed]), "bt_sha1_set_pageable_feed")
    return {v: k for k, v in PAGEABLE_FEEDS.items()}[prev]


def pipeline_stats():
    """Phase times and NUMA placement of this thread's last host pipeline run
    (bt_sha1_get_pipeline_stats) as a dict; per-node tallies are trimmed to
    the machine's node count."""
    s = PipelineStats()
    _check(lib.bt_sha1_get_pipeline_stats(ctypes.byref(s)), "bt_sha1_get_pipeline_stats")
    nodes = max(1, min(STATS_NODES, s.numa_nodes))
    d = {k: getattr(s, k) for k, _ in PipelineStats._fields_}
    for k in ("lane_pages", "src_pages", "copy_pieces"):
        d[k] = list(d[k])[:nodes]
    for k in ("total_s", "alloc_s", "fill_s", "wait_s", "register_s", "unregister_s"):
        d[k] = round(d[k], 4)
    d["feed"] = {0: "direct", 1: "staged", 2: "registered"}.get(s.staged, "?")
    d["staged"], d["numa_policy"] = s.staged == 1, {1: "lanes", 2: "gpu"}.get(s.numa_policy, "none")
    return d


def shahash(data):
    """chunk.h:28 through the GPU (aborts the process on a GPU error, like the C call)."""
    buf, n = _host_buf(data)
    out = (ctypes.c_uint8 * 20)()
    lib.shahash(buf, n, out)
    return bytes(out)


class Sha1:
    """SHA1Init/SHA1Update/SHA1Final (sha.h:58-60) on a caller-owned context."""

    def __init__(self):
        self.ctx = SHA1Context()
        lib.SHA1Init(ctypes.byref(self.ctx))

    def update(self, data):
        buf, n = _host_buf(data)
        lib.SHA1Update(ctypes.byref(self.ctx), buf, n)
        return self

    def final(self):
        out = (ctypes.c_uint8 * 20)()
        lib.SHA1Final(ctypes.byref(self.ctx), out)
        return bytes(out)


def binary2hex(b):
    out = ctypes.create_string_buffer(2 * len(b) + 1)
    lib.binary2hex((ctypes.c_uint8 * max(len(b), 1)).from_buffer_copy(bytes(b) or b"\0"), len(b), out)
    return out.value.decode()


def hex2binary(h):
    hb = h.encode() if isinstance(h, str) else bytes(h)
    out = (ctypes.c_uint8 * max(len(hb) // 2, 1))()
    lib.hex2binary(ctypes.create_string_buffer(hb, len(hb) + 1), len(hb), out)
    return bytes(out)[:len(hb) // 2]


def make_chunks_file(path, chunk_len=CHUNK):
    """bt_sha1_chunks_file over an open FILE* (libc fopen through ctypes)."""
    libc = ctypes.CDLL(None)
    libc.fopen.restype = _vp
    libc.fopen.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    libc.fclose.argtypes = [_vp]
    size = os.path.getsize(path)
    nch = (size + chunk_len - 1) // chunk_len
    out = (ctypes.c_uint8 * max(20 * nch, 1))()
    fp = libc.fopen(path.encode(), b"rb")
    if not fp:
        raise OSError(f"cannot open {path}")
    try:
        got = _check(lib.bt_sha1_chunks_file(fp, chunk_len, out, nch), "bt_sha1_chunks_file")
    finally:
        libc.fclose(fp)
    raw = bytes(out)
    return [raw[20 * i:20 * i + 20] for i in range(got)]


class Verifier:
    """Batched asynchronous verify (bt_sha1_verifier_*).  ragged=True: chunks
    of any length from 1 to chunk_len (bt_sha1_verifier_create_ragged), e.g. a
    file's short last chunk; commit / submit then carry the chunk's own length.
    gather=True: the slots hold datagrams (bt_sha1_verifier_create_gather);
    chunk_len is the slot length, max_segs the most segments commit_gather lists."""

    def __init__(self, device=0, chunk_len=CHUNK, batch=64, nstreams=2, ragged=False, gather=False, max_segs=0):
        if gather:
            self.h = lib.bt_sha1_verifier_create_gather(device, chunk_len, max_segs, batch, nstreams)
        else:
            create = lib.bt_sha1_verifier_create_ragged if ragged else lib.bt_sha1_verifier_create
            self.h = create(device, chunk_len, batch, nstreams)
        if not self.h:
            kind = "_gather" if gather else "_ragged" if ragged else ""
            raise BtSha1Error(f"bt_sha1_verifier_create{kind}: {last_error()}")
        self.chunk_len = chunk_len
        self.ragged = ragged
        self.gather = gather
        self.max_segs = max_segs

    def submit(self, chunk, expected, tag):
        buf, n = _host_buf(chunk)
        e = (ctypes.c_uint8 * 20).from_buffer_copy(bytes(expected))
        _check(lib.bt_sha1_verifier_submit(self.h, buf, n, e, tag), "bt_sha1_verifier_submit")

    def slot(self):
        """Hand out a pinned slot (integer address) to assemble a chunk in."""
        p = lib.bt_sha1_verifier_slot(self.h)
        if not p:
            raise BtSha1Error(f"bt_sha1_verifier_slot: {last_error()}")
        return p

    def commit(self, slot, expected, tag, length=None):
        e = (ctypes.c_uint8 * 20).from_buffer_copy(bytes(expected))
        _check(lib.bt_sha1_verifier_commit(self.h, slot, length or self.chunk_len, e, tag),
               "bt_sha1_verifier_commit")

    def commit_gather(self, slot, segs, expected, tag):
        """Queue the chunk made of segs, a list of (off, len) within the slot, in this order."""
        e = (ctypes.c_uint8 * 20).from_buffer_copy(bytes(expected))
        table = (Seg * max(len(segs), 1))(*[Seg(off, length, 0) for off, length in segs])
        _check(lib.bt_sha1_verifier_commit_gather(self.h, slot, table, len(segs), e, tag),
               "bt_sha1_verifier_commit_gather")

    def release(self, slot):
        _check(lib.bt_sha1_verifier_release(self.h, slot), "bt_sha1_verifier_release")

    def flush(self):
        _check(lib.bt_sha1_verifier_flush(self.h), "bt_sha1_verifier_flush")

    def slot_fill(self, chunk, expected, tag):
        """Zero-copy form: write into a pinned slot, then commit it."""
        p = self.slot()
        ctypes.memmove(p, bytes(chunk), len(chunk))
        self.commit(p, expected, tag, len(chunk))

    def _collect(self, fn, max_n=4096):
        out = (Verdict * max_n)()
        got = _check(fn(self.h, out, max_n), "verifier")
        return [(out[i].tag, bool(out[i].ok), bytes(out[i].digest)) for i in range(got)]

    def poll(self):
        return self._collect(lib.bt_sha1_verifier_poll)

    def drain(self):
        res = []
        while True:
            r = self._collect(lib.bt_sha1_verifier_drain)
            if not r:
                return res
            res += r

    def pending(self):
        return lib.bt_sha1_verifier_pending(self.h)

    def stats(self):
        """bt_sha1_verifier_get_stats as a dict."""
        s = VerifierStats()
        _check(lib.bt_sha1_verifier_get_stats(self.h, ctypes.byref(s)), "bt_sha1_verifier_get_stats")
        return {k: getattr(s, k) for k, _ in VerifierStats._fields_}

    def gather_stats(self):
        """bt_sha1_verifier_get_gather_stats as a dict."""
        s = VerifierGatherStats()
        _check(lib.bt_sha1_verifier_get_gather_stats(self.h, ctypes.byref(s)), "bt_sha1_verifier_get_gather_stats")
        return {k: getattr(s, k) for k, _ in VerifierGatherStats._fields_}

    def close(self):
        if self.h:
            lib.bt_sha1_verifier_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


NEVER = 0xFFFFFFFF  # Receiver stride: nothing is hashed before commit


class Receiver:
    """Progressive receive (bt_sha1_receiver_*): a chunk is hashed while its
    payloads arrive, so commit leaves only the last stride and the padding."""

    def __init__(self, device=0, chunk_len=CHUNK, nslots=4, stride=0):
        self.h = lib.bt_sha1_receiver_create(device, chunk_len, nslots, stride)
        if not self.h:
            raise BtSha1Error(f"bt_sha1_receiver_create: {last_error()}")
        self.chunk_len = chunk_len

    def slot(self):
        """Hand out a pinned slot (integer address) to receive a chunk into, in order."""
        p = lib.bt_sha1_receiver_slot(self.h)
        if not p:
            raise BtSha1Error(f"bt_sha1_receiver_slot: {last_error()}")
        return p

    def advance(self, slot, filled):
        """Bytes [0, filled) of the slot are final."""
        _check(lib.bt_sha1_receiver_advance(self.h, slot, filled), "bt_sha1_receiver_advance")

    def commit(self, slot, expected, tag, length=None):
        e = (ctypes.c_uint8 * 20).from_buffer_copy(bytes(expected))
        _check(lib.bt_sha1_receiver_commit(self.h, slot, self.chunk_len if length is None else length, e, tag),
               "bt_sha1_receiver_commit")

    def release(self, slot):
        _check(lib.bt_sha1_receiver_release(self.h, slot), "bt_sha1_receiver_release")

    def receive(self, chunk, expected, tag, piece=1484):
        """A whole chunk as the peer's receive path delivers it: `piece`-byte
        payloads appended in order (util.c:275), advance after each, commit."""
        p = self.slot()
        data = bytes(chunk)
        for o in range(0, len(data), piece):
            part = data[o:o + piece]
            ctypes.memmove(p + o, part, len(part))
            self.advance(p, o + len(part))
        self.commit(p, expected, tag, len(data))

    def _collect(self, fn, max_n=256):
        out = (Verdict * max_n)()
        got = _check(fn(self.h, out, max_n), "receiver")
        return [(out[i].tag, bool(out[i].ok), bytes(out[i].digest)) for i in range(got)]

    def poll(self):
        return self._collect(lib.bt_sha1_receiver_poll)

    def drain(self):
        res = []
        while True:
            r = self._collect(lib.bt_sha1_receiver_drain)
            if not r:
                return res
            res += r

    def pending(self):
        return lib.bt_sha1_receiver_pending(self.h)

    def stats(self):
        s = ReceiverStats()
        _check(lib.bt_sha1_receiver_get_stats(self.h, ctypes.byref(s)), "bt_sha1_receiver_get_stats")
        return {k: int(getattr(s, k)) for k, _ in ReceiverStats._fields_}

    def close(self):
        if self.h:
            lib.bt_sha1_receiver_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Intake:
    """Progressive receive for many chunks at once (bt_sha1_intake_*): advance
    and commit only record what has arrived, and one kick (poll ends with one)
    advances every due slot in a single launch.

    gather=True (bt_sha1_intake_create_gather): a slot holds datagrams where
    they landed, chunk_len is the slot's length and max_segs the most segments
    a chunk may list; append / commit_gather take the place of advance /
    commit, everything else is the same."""

    def __init__(self, device=0, chunk_len=CHUNK, nslots=64, stride=0, gather=False, max_segs=0):
        self.gather = bool(gather)
        if self.gather:
            self.h = lib.bt_sha1_dgram_slots_create(device, chunk_len, max_segs, nslots, stride)
        else:
            self.h = lib.bt_sha1_intake_create(device, chunk_len, nslots, stride)
        if not self.h:
            raise BtSha1Error(f"bt_sha1_intake_create{'_gather' if self.gather else ''}: {last_error()}")
        self.chunk_len = chunk_len
        self.nslots = nslots

    def slot(self):
        """Hand out a pinned slot (integer address) to receive a chunk into, in order."""
        p = lib.bt_sha1_intake_slot(self.h)
        if not p:
            raise BtSha1Error(f"bt_sha1_intake_slot: {last_error()}")
        return p

    def advance(self, slot, filled):
        """Bytes [0, filled) of the slot are final (recorded; nothing is launched)."""
        _check(lib.bt_sha1_intake_advance(self.h, slot, filled), "bt_sha1_intake_advance")

    def commit(self, slot, expected, tag, length=None):
        e = (ctypes.c_uint8 * 20).from_buffer_copy(bytes(expected))
        _check(lib.bt_sha1_intake_commit(self.h, slot, self.chunk_len if length is None else length, e, tag),
               "bt_sha1_intake_commit")

    def append(self, slot, segs):
        """The next payload segments in sequence order, (off, len) pairs relative to the slot (recorded only)."""
        arr = (Seg * max(len(segs), 1))()
        for k, (off, length) in enumerate(segs):
            arr[k].off, arr[k].len = off, length
        _check(lib.bt_sha1_dgram_slots_append(self.h, slot, arr, len(segs)), "bt_sha1_intake_append")

    def commit_gather(self, slot, expected, tag):
        """The chunk is complete at the bytes listed."""
        e = (ctypes.c_uint8 * 20).from_buffer_copy(bytes(expected))
        _check(lib.bt_sha1_dgram_slots_commit(self.h, slot, e, tag), "bt_sha1_intake_commit_gather")

    def receive_datagrams(self, chunk, order, expected, tag, payload=1484, header=16, each=None):
        """One whole chunk as DATA datagrams (a `header`-byte header that
        starts with the sequence number, then up to `payload` bytes) that
        arrive in `order`, a list of sequence numbers in which every one occurs
        and duplicates may: each lands where the last one ended, a duplicate
        is never listed, and a payload is appended once the gap before it has
        filled, together with those held back behind it.  each(slot), when
        given, runs after every append (a test kicks there).  Then
        commit_gather (no kick).  Returns the slot."""
        data = bytes(chunk)
        p = self.slot()
        where, listed = {}, 0
        for arrival, seq in enumerate(order):
            part = data[seq * payload:(seq + 1) * payload]
            at = arrival * (header + payload)
            pkt = int(seq).to_bytes(4, "little") + bytes(header - 4) + part
            ctypes.memmove(p + at, pkt, len(pkt))
            where.setdefault(seq, (at + header, len(part)))
            ready = []
            while listed in where:
                ready.append(where[listed])
                listed += 1
            if ready:
                self.append(p, ready)
                if each:
                    each(p)
        self.commit_gather(p, expected, tag)
        return p

    def release(self, slot):
        _check(lib.bt_sha1_intake_release(self.h, slot), "bt_sha1_intake_release")

    def kick(self):
        """One launch for every due slot with no launch in flight; the entries launched."""
        return _check(lib.bt_sha1_intake_kick(self.h), "bt_sha1_intake_kick")

    def sync(self):
        """Wait for every queued launch; launches nothing."""
        _check(lib.bt_sha1_intake_sync(self.h), "bt_sha1_intake_sync")

    def receive(self, chunk, expected, tag, piece=1484):
        """One whole chunk: `piece`-byte payloads in order, advance after each, commit (no kick)."""
        p = self.slot()
        data = bytes(chunk)
        for o in range(0, len(data), piece):
            part = data[o:o + piece]
            ctypes.memmove(p + o, part, len(part))
            self.advance(p, o + len(part))
        self.commit(p, expected, tag, len(data))

    def receive_all(self, chunks, expected, tags, piece=1484):
        """All the chunks as an event loop with many downloads delivers them:
        every turn each chunk in progress gets one `piece`-byte payload in its
        slot (advance), a complete chunk is committed, and the turn ends with
        ONE poll.  More chunks than slots wait for a slot.  Returns every
        verdict."""
        chunks = [bytes(c) for c in chunks]
        waiting = list(range(len(chunks)))
        active, got = [], []  # active: [chunk index, slot, bytes delivered]
        while waiting or active:
            while waiting and len(active) < self.nslots:
                try:
                    p = self.slot()
                except BtSha1Error:
                    break  # every slot is receiving or waits for its verdict: next turn
                active.append([waiting.pop(0), p, 0])
            still = []
            for a in active:
                k, p, o = a
                part = chunks[k][o:o + piece]
                ctypes.memmove(p + o, part, len(part))
                a[2] = o + len(part)
                self.advance(p, a[2])
                if a[2] == len(chunks[k]):
                    self.commit(p, expected[k], tags[k], a[2])
                else:
                    still.append(a)
            active = still
            # nothing left to deliver until a slot comes back: wait for the verdicts instead of polling in a loop
            got += self.poll() if active or not waiting else self.drain()
        return got + self.drain()

    def _collect(self, fn, max_n=512):
        out = (Verdict * max_n)()
        got = _check(fn(self.h, out, max_n), "intake")
        return [(out[i].tag, bool(out[i].ok), bytes(out[i].digest)) for i in range(got)]

    def poll(self):
        return self._collect(lib.bt_sha1_intake_poll)

    def drain(self):
        res = []
        while True:
            r = self._collect(lib.bt_sha1_intake_drain)
            if not r:
                return res
            res += r

    def pending(self):
        return lib.bt_sha1_intake_pending(self.h)

    def stats(self):
        s = IntakeStats()
        _check(lib.bt_sha1_intake_get_stats(self.h, ctypes.byref(s)), "bt_sha1_intake_get_stats")
        return {k: int(getattr(s, k)) for k, _ in IntakeStats._fields_}

    def close(self):
        if self.h:
            lib.bt_sha1_intake_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

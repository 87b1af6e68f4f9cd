"""ctypes binding of libsdcas.so (include/sdcas.h, include/sdcas_bench.h).

The library is the product: every hash and every dedup result comes from its
HIP kernels. Importing this module without the built library, or calling it
without a GPU, raises — there is no CPU fallback.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsdcas.so")

SDCAS_OK = 0
SDCAS_E_NO_DEVICE = -1
SDCAS_E_INVALID = -2
SDCAS_E_OOM = -3
SDCAS_E_HIP = -4
SDCAS_E_CAPACITY = -5
SDCAS_E_CANCELLED = -6
SDCAS_STATUS_UNEXPECTED_EOF = 100001
SDCAS_STATUS_CANCELLED = 125
SDCAS_MAX_BATCH = 0x7FFFFFFF
SDCAS_OPT_DIRECT_IO = 1
SDCAS_ABI_VERSION = 7
SDCAS_META_HAS_CAS_ID = 1
SDCAS_META_DIR = 2
SDCAS_META_HAS_CHECKSUM = 4
SDCAS_LINK_DROPPED = -(1 << 63)
SDCAS_LINK_DEFERRED = SDCAS_LINK_DROPPED + 1
SDCAS_PLAN_HEADER_WORDS = 12
SDCAS_CONFIRM_DUPLICATE = 1
SDCAS_CONFIRM_COLLISION = 2
SDCAS_CONFIRM_SKIPPED = 4
SDCAS_SETS_BY_REP = 0
SDCAS_SETS_BY_RECLAIMABLE = 1
SDCAS_TREE_MAX_DEPTH = 4096
SDCAS_TREE_DIR = 1
SDCAS_TREE_INCOMPLETE = 2
SDCAS_TREE_EMPTY = 4
SDCAS_TOP_DUP = 1
SDCAS_TOP_NESTED = 2
SDCAS_CHUNK_PARAMS_DEFAULT = (2048, 13, 65536)
SDCAS_CHUNK_MAX_CHUNKS = 1 << 30
SDCAS_CHUNK_GEAR_TILE = 32768
SDCAS_CHUNK_GEAR_STRIP = 128
SDCAS_INDEX_MAX_ENTRIES = 1 << 30
SDCAS_INDEX_MAX_BITS = 28
SDCAS_INDEX_HIT = 1
SDCAS_INDEX_ADDED = 2
SDCAS_INDEX_SKIPPED = 4
SDCAS_PEERS_EARLIER = 0
SDCAS_PEERS_ALL = 1
SDCAS_PEERS_MAX_K = 64
SDCAS_PEERS_MAX_HOLDERS = 1 << 20
SDCAS_PEERS_MAX_PAIRS = 1 << 30

# every entry point include/sdcas.h and include/sdcas_bench.h declare
ABI_SYMBOLS = [
    "sdcas_version", "sdcas_abi_version", "sdcas_init", "sdcas_destroy", "sdcas_last_error", "sdcas_cas_ids",
    "sdcas_file_metadata", "sdcas_identify_checksums", "sdcas_dev_identify",
    "sdcas_checksums", "sdcas_hash_messages", "sdcas_cas_ids_from_messages", "sdcas_dev_reserve",
    "sdcas_dev_hash_messages", "sdcas_dev_sync", "sdcas_dev_bind_stream", "sdcas_dedup", "sdcas_dedup_window", "sdcas_job_plan",
    "sdcas_confirm_duplicates", "sdcas_dev_confirm_duplicates",  # added after ABI 7
    "sdcas_duplicate_sets", "sdcas_dev_duplicate_sets",  # added after ABI 7
    "sdcas_tree_plan", "sdcas_tree_digests", "sdcas_dev_tree_digests", "sdcas_tree_top",
    "sdcas_dev_tree_top",  # added after ABI 7
    "sdcas_chunk_plan", "sdcas_chunk_messages", "sdcas_dev_chunk", "sdcas_chunk_sharing",
    "sdcas_dev_chunk_sharing",  # added after ABI 7
    "sdcas_chunk_seg_bytes", "sdcas_chunk_windows", "sdcas_dev_chunk_windows",  # added after ABI 7
    "sdcas_chunk_index_dir_bits", "sdcas_chunk_index_check", "sdcas_chunk_index_match",
    "sdcas_dev_chunk_index_match", "sdcas_chunk_index_add", "sdcas_dev_chunk_index_add",  # added after ABI 7
    "sdcas_chunk_holders_check", "sdcas_chunk_holders_match", "sdcas_dev_chunk_holders_match",
    "sdcas_chunk_holders_add", "sdcas_dev_chunk_holders_add", "sdcas_chunk_holders_remove",
    "sdcas_dev_chunk_holders_remove",  # added after ABI 7
    "sdcas_chunk_peers_plan", "sdcas_chunk_peers", "sdcas_dev_chunk_peers",  # added after ABI 7
    "sdcas_file_families_plan", "sdcas_file_families", "sdcas_dev_file_families",  # added after ABI 7
    "sdcas_family_bytes_plan", "sdcas_family_bytes", "sdcas_dev_family_bytes",  # added after ABI 7
    "sdcas_family_recipes_plan", "sdcas_family_recipes", "sdcas_dev_family_recipes",  # added after ABI 7
    "sdcas_family_store_tile_bytes", "sdcas_family_store_plan", "sdcas_family_store_layout", "sdcas_family_pack",
    "sdcas_family_restore", "sdcas_dev_family_store_layout", "sdcas_dev_family_pack",
    "sdcas_dev_family_restore",  # added after ABI 7
    "sdcas_family_forget_plan", "sdcas_family_chunks_keep", "sdcas_dev_family_chunks_keep",
    "sdcas_family_store_moves", "sdcas_dev_family_store_moves",  # added after ABI 7
    "sdcas_key_to_hex",
    "sdcas_digest_to_hex", "sdcas_cas_message_len", "sdcas_dev_dedup_combine", "sdcas_dev_dedup_combine_async",
    "sdcas_dev_dedup_resolve",
    "sdcas_dev_dedup_apply", "sdcas_dev_dedup_local", "sdcas_dev_dedup_combine_buckets",
    "sdcas_dev_dedup_resolve_buckets", "sdcas_dev_dedup_stays", "sdcas_dev_dedup_plan", "sdcas_dev_stream_begin", "sdcas_dev_stream_update",
    "sdcas_dev_stream_finish", "sdcas_dev_stream_node_bytes", "sdcas_dev_stream_export", "sdcas_dev_stream_import",
    "sdcas_set_progress", "sdcas_node_init", "sdcas_node_destroy", "sdcas_node_last_error", "sdcas_node_size",
    "sdcas_node_uses_rccl", "sdcas_node_set_progress", "sdcas_node_cas_ids", "sdcas_node_checksums",
    "sdcas_node_dedup_window",
    # bench / test plumbing
    "sdcas_dev_synth_cas_messages", "sdcas_dev_synth_content", "sdcas_dev_dedup", "sdcas_dev_profile",
    "sdcas_dev_last_kernel_ms", "sdcas_dev_set_leaf_variant", "sdcas_dev_set_piece_variant", "sdcas_dev_set_sort",
]


class SdcasError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"sdcas error {code}: {msg}")
        self.code = code


class Cancelled(SdcasError):
    """SDCAS_E_CANCELLED: the call stopped at the cancel flag. `partial` holds
    what the call returns normally (results and per-item status); items with
    status SDCAS_STATUS_CANCELLED were not completed, the others are final."""

    def __init__(self, msg, partial=None):
        super().__init__(SDCAS_E_CANCELLED, msg)
        self.partial = partial


# void (*)(void* user, uint64_t done, uint64_t total)
PROGRESS_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64)


class Options(ctypes.Structure):
    """sdcas_options; struct_size is set to this layout's size"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("device", ctypes.c_int32), ("io_threads", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("staging_bytes", ctypes.c_uint64),
                ("progress", PROGRESS_FN),
                ("progress_user", ctypes.c_void_p), ("cancel", ctypes.POINTER(ctypes.c_int32))]

    def __init__(self, *a, **k):
        super().__init__(ctypes.sizeof(Options), *a, **k)


class JobWindow(ctypes.Structure):
    """sdcas_job_window"""
    _fields_ = [("max_steps", ctypes.c_uint64), ("more", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("steps", ctypes.c_uint64), ("rows", ctypes.c_uint64), ("rereads", ctypes.c_uint64)]


class ConfirmCounts(ctypes.Structure):
    """sdcas_confirm_counts"""
    _fields_ = [("files", ctypes.c_uint64), ("classes", ctypes.c_uint64), ("keys", ctypes.c_uint64),
                ("collided_keys", ctypes.c_uint64), ("collided_files", ctypes.c_uint64),
                ("duplicate_files", ctypes.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class SetsCounts(ctypes.Structure):
    """sdcas_sets_counts"""
    _fields_ = [("files", ctypes.c_uint64), ("sets", ctypes.c_uint64), ("members", ctypes.c_uint64),
                ("duplicate_files", ctypes.c_uint64), ("reclaimable_bytes", ctypes.c_uint64),
                ("largest_set", ctypes.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class TreeCounts(ctypes.Structure):
    """sdcas_tree_counts"""
    _fields_ = [("entries", ctypes.c_uint64), ("dirs", ctypes.c_uint64), ("complete_dirs", ctypes.c_uint64),
                ("empty_dirs", ctypes.c_uint64), ("levels", ctypes.c_uint64), ("largest_dir", ctypes.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class TopCounts(ctypes.Structure):
    """sdcas_top_counts"""
    _fields_ = [("entries", ctypes.c_uint64), ("dup_entries", ctypes.c_uint64), ("nested_entries", ctypes.c_uint64),
                ("top_entries", ctypes.c_uint64), ("kept_classes", ctypes.c_uint64),
                ("dropped_classes", ctypes.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class ChunkParams(ctypes.Structure):
    """sdcas_chunk_params"""
    _fields_ = [("min_len", ctypes.c_uint32), ("avg_bits", ctypes.c_uint32), ("max_len", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class ChunkCounts(ctypes.Structure):
    """sdcas_chunk_counts"""
    _fields_ = [("files", ctypes.c_uint64), ("chunks", ctypes.c_uint64), ("total_bytes", ctypes.c_uint64),
                ("hash_cuts", ctypes.c_uint64), ("max_cuts", ctypes.c_uint64), ("end_chunks", ctypes.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class SharingCounts(ctypes.Structure):
    """sdcas_sharing_counts"""
    _fields_ = [("files", ctypes.c_uint64), ("chunks", ctypes.c_uint64), ("distinct_chunks", ctypes.c_uint64),
                ("total_bytes", ctypes.c_uint64), ("stored_bytes", ctypes.c_uint64),
                ("files_with_peer", ctypes.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class IndexMatchCounts(ctypes.Structure):
    """sdcas_index_match_counts"""
    _fields_ = [("queries", ctypes.c_uint64), ("hits", ctypes.c_uint64), ("misses", ctypes.c_uint64),
                ("skipped", ctypes.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class IndexAddCounts(ctypes.Structure):
    """sdcas_index_add_counts"""
    _fields_ = [("queries", ctypes.c_uint64), ("hits", ctypes.c_uint64), ("added", ctypes.c_uint64),
                ("batch_duplicates", ctypes.c_uint64), ("entries_old", ctypes.c_uint64),
                ("entries_new", ctypes.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class HoldersRemoveCounts(ctypes.Structure):
    """sdcas_holders_remove_counts"""
    _fields_ = [("entries_old", ctypes.c_uint64), ("removed", ctypes.c_uint64), ("entries_new", ctypes.c_uint64),
                ("values", ctypes.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class PeersCounts(ctypes.Structure):
    """sdcas_peers_counts"""
    _fields_ = [("files", ctypes.c_uint64), ("chunks", ctypes.c_uint64), ("common_chunks", ctypes.c_uint64),
                ("pairs", ctypes.c_uint64), ("edges", ctypes.c_uint64), ("files_with_peer", ctypes.c_uint64),
                ("overflow", ctypes.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class FamiliesCounts(ctypes.Structure):
    """sdcas_families_counts"""
    _fields_ = [("files", ctypes.c_uint64), ("slots", ctypes.c_uint64), ("missing", ctypes.c_uint64),
                ("self_slots", ctypes.c_uint64), ("weak", ctypes.c_uint64), ("links", ctypes.c_uint64),
                ("families", ctypes.c_uint64), ("members", ctypes.c_uint64), ("largest", ctypes.c_uint64),
                ("unsorted", ctypes.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class FamilyBytesCounts(ctypes.Structure):
    """sdcas_family_bytes_counts"""
    _fields_ = [("files", ctypes.c_uint64), ("chunks", ctypes.c_uint64), ("classes", ctypes.c_uint64),
                ("total_bytes", ctypes.c_uint64), ("stored_bytes", ctypes.c_uint64), ("sets", ctypes.c_uint64),
                ("members", ctypes.c_uint64), ("set_reclaimable_bytes", ctypes.c_uint64),
                ("largest_reclaimable", ctypes.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class FamilyRecipesCounts(ctypes.Structure):
    """sdcas_family_recipes_counts"""
    _fields_ = [("files", ctypes.c_uint64), ("chunks", ctypes.c_uint64), ("ops", ctypes.c_uint64),
                ("literal_ops", ctypes.c_uint64), ("copy_ops", ctypes.c_uint64), ("literal_bytes", ctypes.c_uint64),
                ("copy_bytes", ctypes.c_uint64), ("longest_op", ctypes.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class FamilyStoreCounts(ctypes.Structure):
    """sdcas_family_store_counts"""
    _fields_ = [("ops", ctypes.c_uint64), ("literal_ops", ctypes.c_uint64), ("copy_ops", ctypes.c_uint64),
                ("uncovered_ops", ctypes.c_uint64), ("store_bytes", ctypes.c_uint64),
                ("uncovered_bytes", ctypes.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class FamilyMoveCounts(ctypes.Structure):
    """sdcas_family_move_counts"""
    _fields_ = [("ops_moved", ctypes.c_uint64), ("bytes_moved", ctypes.c_uint64), ("bad_ops", ctypes.c_uint64),
                ("tiles", ctypes.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class FamilyKeepCounts(ctypes.Structure):
    """sdcas_family_keep_counts"""
    _fields_ = [("rows_kept", ctypes.c_uint64), ("rows_removed", ctypes.c_uint64), ("chunks_kept", ctypes.c_uint64),
                ("chunks_removed", ctypes.c_uint64), ("bytes_kept", ctypes.c_uint64),
                ("bytes_removed", ctypes.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class FamilyMovesCounts(ctypes.Structure):
    """sdcas_family_moves_counts"""
    _fields_ = [("moves", ctypes.c_uint64), ("literal_chunks", ctypes.c_uint64), ("moved_bytes", ctypes.c_uint64),
                ("lost_chunks", ctypes.c_uint64), ("lost_bytes", ctypes.c_uint64), ("longest_move", ctypes.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


_lib = None
_lib_path = LIB_PATH


_vp = ctypes.c_void_p
_sz = ctypes.c_size_t
_u64 = ctypes.c_uint64


def load():
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch-ROCm bundles its own
    # libamdhip64.so.7 / libhsa-runtime64.so.1 (same SONAMEs as /opt/rocm's).
    # If torch is importable it is loaded FIRST so that the dynamic linker
    # binds libsdcas.so to torch's already-loaded runtime instead of opening
    # a second HSA runtime on the same GPU (which leaves torch with "No HIP
    # GPUs are available"). Without torch, /opt/rocm's runtime is used.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(_lib_path):
        raise ImportError(f"{_lib_path} is not built: run `make -C spacedrive_amd/csrc` "
                          "(or __graft_entry__.build()) — there is no CPU fallback")
    L = ctypes.CDLL(_lib_path)
    L.sdcas_version.restype = ctypes.c_char_p
    L.sdcas_abi_version.restype = ctypes.c_int
    if L.sdcas_abi_version() != SDCAS_ABI_VERSION:
        raise ImportError(f"{_lib_path} has C ABI {L.sdcas_abi_version()}, this binding {SDCAS_ABI_VERSION}: rebuild")
    L.sdcas_init.argtypes = [ctypes.POINTER(Options), ctypes.POINTER(_vp)]
    L.sdcas_destroy.argtypes = [_vp]
    L.sdcas_last_error.argtypes = [_vp]
    L.sdcas_last_error.restype = ctypes.c_char_p
    L.sdcas_cas_ids.argtypes = [_vp, _vp, _vp, _sz, _vp, _vp]
    L.sdcas_file_metadata.argtypes = [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp]
    L.sdcas_identify_checksums.argtypes = [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp]
    L.sdcas_dev_identify.argtypes = [_vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp]
    L.sdcas_checksums.argtypes = [_vp, _vp, _sz, _vp, _vp]
    L.sdcas_hash_messages.argtypes = [_vp, _vp, _vp, _vp, _sz, _vp]
    L.sdcas_cas_ids_from_messages.argtypes = [_vp, _vp, _vp, _vp, _sz, _vp]
    L.sdcas_dev_reserve.argtypes = [_vp, _sz, _u64]
    L.sdcas_dev_hash_messages.argtypes = [_vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp]
    L.sdcas_dev_sync.argtypes = [_vp, _vp]
    L.sdcas_dev_bind_stream.argtypes = [_vp, _vp, ctypes.c_uint64]
    L.sdcas_dedup.argtypes = [_vp, _vp, _vp, _vp, _sz, _sz, _vp, _sz, _vp, _vp, _vp]
    L.sdcas_job_plan.argtypes = [_vp, _vp, _sz, _sz, ctypes.POINTER(JobWindow), _vp, _vp]
    L.sdcas_dedup_window.argtypes = [_vp, _vp, _vp, _vp, _sz, _sz, _vp, _sz, ctypes.POINTER(JobWindow), _vp, _vp,
                                     _vp]
    L.sdcas_confirm_duplicates.argtypes = [_vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, ctypes.POINTER(ConfirmCounts)]
    L.sdcas_dev_confirm_duplicates.argtypes = [_vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp]
    L.sdcas_duplicate_sets.argtypes = [_vp, _vp, _vp, _sz, ctypes.c_uint32, _vp, _vp, _vp, _vp,
                                       ctypes.POINTER(SetsCounts)]
    L.sdcas_dev_duplicate_sets.argtypes = [_vp, _vp, _vp, _sz, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp]
    L.sdcas_tree_plan.argtypes = [_vp, _vp, _sz, _vp, _vp, _vp]
    L.sdcas_tree_digests.argtypes = [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp,
                                     ctypes.POINTER(TreeCounts)]
    L.sdcas_dev_tree_digests.argtypes = [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
    L.sdcas_tree_top.argtypes = [_vp, _vp, _vp, _sz, _vp, _vp, ctypes.POINTER(TopCounts)]
    L.sdcas_dev_tree_top.argtypes = [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp]
    L.sdcas_chunk_plan.argtypes = [_vp, _sz, ctypes.POINTER(ChunkParams), _vp, _vp]
    L.sdcas_chunk_messages.argtypes = [_vp, _vp, _vp, _vp, _sz, ctypes.POINTER(ChunkParams), _vp, _vp, _vp, _vp, _vp,
                                       _vp, ctypes.POINTER(ChunkCounts)]
    L.sdcas_dev_chunk.argtypes = [_vp, _vp, _vp, _vp, _sz, ctypes.POINTER(ChunkParams), _u64, _u64, _vp, _vp, _vp,
                                  _vp, _vp, _vp, _vp, _vp]
    L.sdcas_chunk_seg_bytes.argtypes = [ctypes.POINTER(ChunkParams)]
    L.sdcas_chunk_seg_bytes.restype = _u64
    L.sdcas_chunk_windows.argtypes = [_vp, _vp, _vp, _vp, _vp, _sz, ctypes.POINTER(ChunkParams), _vp, _vp, _vp, _vp,
                                      _vp, _vp, _vp, ctypes.POINTER(ChunkCounts)]
    L.sdcas_dev_chunk_windows.argtypes = [_vp, _vp, _vp, _vp, _vp, _sz, ctypes.POINTER(ChunkParams), _u64, _u64, _vp,
                                          _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
    L.sdcas_chunk_sharing.argtypes = [_vp, _vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _vp,
                                      ctypes.POINTER(SharingCounts)]
    L.sdcas_dev_chunk_sharing.argtypes = [_vp, _vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
    _u32 = ctypes.c_uint32
    L.sdcas_chunk_index_dir_bits.argtypes = [_u64]
    L.sdcas_chunk_index_dir_bits.restype = _u32
    L.sdcas_chunk_index_check.argtypes = [_vp, _vp, _vp, _u64, _u32, _vp]
    L.sdcas_chunk_index_match.argtypes = [_vp, _vp, _vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _sz, _vp, _vp,
                                          ctypes.POINTER(IndexMatchCounts)]
    L.sdcas_dev_chunk_index_match.argtypes = [_vp, _vp, _vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _sz, _vp, _vp, _vp,
                                              _vp]
    L.sdcas_chunk_index_add.argtypes = [_vp, _vp, _vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp,
                                        _vp, _u32, _vp, _vp, ctypes.POINTER(IndexAddCounts)]
    L.sdcas_dev_chunk_index_add.argtypes = [_vp, _vp, _vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _vp, _sz, _vp, _vp,
                                            _vp, _vp, _u32, _vp, _vp, _vp, _vp]
    L.sdcas_chunk_holders_check.argtypes = [_vp, _vp, _vp, _vp, _u64, _u32, _vp]
    L.sdcas_chunk_holders_match.argtypes = [_vp, _vp, _vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _sz, _vp, _vp, _vp,
                                            ctypes.POINTER(IndexMatchCounts)]
    L.sdcas_dev_chunk_holders_match.argtypes = [_vp, _vp, _vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _sz, _vp, _vp,
                                                _vp, _vp, _vp]
    L.sdcas_chunk_holders_add.argtypes = L.sdcas_chunk_index_add.argtypes
    L.sdcas_dev_chunk_holders_add.argtypes = L.sdcas_dev_chunk_index_add.argtypes
    L.sdcas_chunk_holders_remove.argtypes = [_vp, _vp, _vp, _vp, _vp, _u64, _u32, _vp, _sz, _vp, _vp, _vp, _vp, _u32,
                                             ctypes.POINTER(HoldersRemoveCounts)]
    L.sdcas_dev_chunk_holders_remove.argtypes = [_vp, _vp, _vp, _vp, _vp, _u64, _u32, _vp, _sz, _vp, _vp, _vp, _vp,
                                                 _u32, _vp, _vp]
    L.sdcas_chunk_peers_plan.argtypes = [_u64, _u64, _u32, _u32, _vp, _vp]
    L.sdcas_chunk_peers.argtypes = [_vp, _vp, _vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _sz, _u32,
                                    _u32, _u32, _u64, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(PeersCounts)]
    L.sdcas_dev_chunk_peers.argtypes = [_vp, _vp, _vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _sz,
                                        _u32, _u32, _u32, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
    L.sdcas_file_families_plan.argtypes = [_u64, _u32, _vp]
    L.sdcas_file_families.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _u32, _u32, _u32, _vp, _vp,
                                      ctypes.POINTER(FamiliesCounts)]
    L.sdcas_dev_file_families.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _u32, _u32, _u32, _vp, _vp, _vp, _vp]
    L.sdcas_family_bytes_plan.argtypes = [_u64, _u64, _vp]
    L.sdcas_family_bytes.argtypes = [_vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                     ctypes.POINTER(FamilyBytesCounts)]
    L.sdcas_dev_family_bytes.argtypes = [_vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                         _vp]
    L.sdcas_family_recipes_plan.argtypes = [_u64, _u64, _vp]
    L.sdcas_family_recipes.argtypes = [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _sz] + [_vp] * 10 + [
        ctypes.POINTER(FamilyRecipesCounts)]
    L.sdcas_dev_family_recipes.argtypes = [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _sz] + [_vp] * 12
    L.sdcas_family_store_tile_bytes.argtypes = []
    L.sdcas_family_store_tile_bytes.restype = _u64
    L.sdcas_family_store_plan.argtypes = [_u64, _u64, _vp]
    L.sdcas_dev_family_store_layout.argtypes = [_vp] * 9 + [_sz, _vp, _sz, _vp, _vp, _vp]
    L.sdcas_dev_family_pack.argtypes = [_vp] * 8 + [_sz, _vp, _vp, _vp, _sz, _vp, _u64, _vp, _u64, _vp, _vp]
    L.sdcas_dev_family_restore.argtypes = [_vp] * 6 + [_sz, _vp, _vp, _vp, _sz, _vp, _u64, _vp, _u64, _vp, _vp]
    L.sdcas_family_store_layout.argtypes = [_vp] * 8 + [_sz, _vp, _sz, _vp, ctypes.POINTER(FamilyStoreCounts)]
    L.sdcas_family_pack.argtypes = [_vp] * 7 + [_sz, _vp, _vp, _vp, _sz, _vp, _u64, _vp, _u64,
                                                ctypes.POINTER(FamilyMoveCounts)]
    L.sdcas_family_restore.argtypes = [_vp] * 5 + [_sz, _vp, _vp, _vp, _sz, _vp, _u64, _vp, _u64,
                                                   ctypes.POINTER(FamilyMoveCounts)]
    L.sdcas_family_forget_plan.argtypes = [_u64, _u64, _vp]
    L.sdcas_family_chunks_keep.argtypes = [_vp] * 5 + [_sz, _vp, _vp, _sz] + [_vp] * 8 + [
        ctypes.POINTER(FamilyKeepCounts)]
    L.sdcas_dev_family_chunks_keep.argtypes = [_vp] * 5 + [_sz, _vp, _vp, _sz] + [_vp] * 10
    L.sdcas_family_store_moves.argtypes = [_vp, _vp, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp,
                                           _vp, _sz, _vp, _vp, _vp, ctypes.POINTER(FamilyMovesCounts)]
    L.sdcas_dev_family_store_moves.argtypes = [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz,
                                               _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp]
    L.sdcas_key_to_hex.argtypes = [_u64, ctypes.c_char_p]
    L.sdcas_digest_to_hex.argtypes = [_vp, ctypes.c_char_p]
    L.sdcas_cas_message_len.argtypes = [_u64]
    L.sdcas_cas_message_len.restype = _u64
    L.sdcas_dev_synth_cas_messages.argtypes = [_vp, _vp, _vp, _vp, _sz, _vp, _vp]
    L.sdcas_dev_synth_content.argtypes = [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]
    L.sdcas_dev_dedup.argtypes = [_vp, _vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp]
    L.sdcas_dev_profile.argtypes = [_vp, ctypes.c_int]
    L.sdcas_dev_last_kernel_ms.argtypes = [_vp, ctypes.POINTER(ctypes.c_float),
                                           ctypes.POINTER(ctypes.c_float)]
    L.sdcas_dev_set_leaf_variant.argtypes = [_vp, ctypes.c_int]
    L.sdcas_dev_set_piece_variant.argtypes = [_vp, ctypes.c_int]
    L.sdcas_dev_set_sort.argtypes = [_vp, ctypes.c_int]
    L.sdcas_set_progress.argtypes = [_vp, PROGRESS_FN, _vp, ctypes.POINTER(ctypes.c_int32)]
    L.sdcas_dev_dedup_combine_buckets.argtypes = [_vp, _vp, _vp, _vp, _vp, _sz, ctypes.c_uint32, _sz, _vp, _vp,
                                                  _vp, _vp, _vp]
    L.sdcas_dev_dedup_resolve_buckets.argtypes = [_vp, _vp, _sz, _vp, _vp, _sz, _vp, ctypes.c_uint32, _vp, _vp]
    L.sdcas_dev_dedup_combine.argtypes = [_vp, _vp, _vp, _vp, _vp, _sz, ctypes.c_uint32, _vp, _vp, _vp, _vp]
    L.sdcas_dev_dedup_combine_async.argtypes = [_vp, _vp, _vp, _vp, _vp, _sz, ctypes.c_uint32, _vp, _vp, _vp, _vp]
    L.sdcas_dev_dedup_resolve.argtypes = [_vp, _vp, _sz, _vp, _sz, _vp, _vp]
    L.sdcas_dev_dedup_apply.argtypes = [_vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp]
    L.sdcas_dev_dedup_local.argtypes = [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _sz, _sz, _u64, _u64,
                                        ctypes.c_uint32, _vp, _vp, _vp, _vp]
    L.sdcas_dev_dedup_stays.argtypes = [_vp, _vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp]
    L.sdcas_dev_dedup_plan.argtypes = [_vp, _vp, _sz, _u64, _sz, _u64, ctypes.c_uint32, _vp, _vp]
    L.sdcas_dev_stream_begin.argtypes = [_vp, _vp, _sz]
    L.sdcas_dev_stream_update.argtypes = [_vp, _sz, _vp, _vp, _vp, _vp, _vp]
    L.sdcas_dev_stream_finish.argtypes = [_vp, _vp, _vp]
    L.sdcas_dev_stream_node_bytes.argtypes = [_vp]
    L.sdcas_dev_stream_node_bytes.restype = _sz
    L.sdcas_dev_stream_export.argtypes = [_vp, _vp, _sz, _vp]
    L.sdcas_dev_stream_import.argtypes = [_vp, _vp, _sz, _vp]
    L.sdcas_node_init.argtypes = [_vp, _sz, ctypes.POINTER(Options), ctypes.POINTER(_vp)]
    L.sdcas_node_destroy.argtypes = [_vp]
    L.sdcas_node_last_error.argtypes = [_vp]
    L.sdcas_node_last_error.restype = ctypes.c_char_p
    L.sdcas_node_size.argtypes = [_vp]
    L.sdcas_node_size.restype = _sz
    L.sdcas_node_uses_rccl.argtypes = [_vp]
    L.sdcas_node_set_progress.argtypes = [_vp, PROGRESS_FN, _vp, ctypes.POINTER(ctypes.c_int32)]
    L.sdcas_node_cas_ids.argtypes = [_vp, _vp, _vp, _sz, _vp, _vp]
    L.sdcas_node_checksums.argtypes = [_vp, _vp, _sz, _vp, _vp]
    L.sdcas_node_dedup_window.argtypes = [_vp, _vp, _vp, _vp, _sz, _sz, _vp, _sz, ctypes.POINTER(JobWindow), _vp,
                                          _vp, _vp]
    _lib = L
    return L

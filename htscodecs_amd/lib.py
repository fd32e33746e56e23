"""ctypes binding of librans4x16_hip.so (include/rans4x16_hip.h)."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# R4X16_LIB: another build of the SAME library (tools/build_variant.sh -> htscodecs_amd/variants/lib<name>.so) for A/B
# measurements; it must exist and export the whole ABI, there is no fallback either way.
LIB_PATH = os.environ.get("R4X16_LIB") or os.path.join(_HERE, "librans4x16_hip.so")

STATUS_NAMES = {0: "OK", 1: "CAPACITY", 2: "TRUNCATED", 3: "TABLE", 4: "STATE", 5: "SIZE",
                6: "UNSUPPORTED", 7: "CONTEXT", 8: "RLE", 9: "EMPTY"}

# name -> (restype, argtypes); the single source of truth that tests/test_cabi.py checks against
# the declarations in include/rans4x16_hip.h.
_u8p = C.c_void_p
SIGNATURES = {
    "rans_compress_bound_4x16": (C.c_uint, [C.c_uint, C.c_int]),
    "rans_compress_to_4x16": (C.c_void_p, [_u8p, C.c_uint, _u8p, C.POINTER(C.c_uint), C.c_int]),
    "rans_compress_4x16": (C.c_void_p, [_u8p, C.c_uint, C.POINTER(C.c_uint), C.c_int]),
    "rans_uncompress_to_4x16": (C.c_void_p, [_u8p, C.c_uint, _u8p, C.POINTER(C.c_uint)]),
    "rans_uncompress_4x16": (C.c_void_p, [_u8p, C.c_uint, C.POINTER(C.c_uint)]),
    "rans4x16_hip_create": (C.c_void_p, [C.c_int]),
    "rans4x16_hip_destroy": (None, [C.c_void_p]),
    "rans4x16_hip_last_error": (C.c_char_p, [C.c_void_p]),
    "rans4x16_hip_compress_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p]),
    "rans4x16_hip_uncompress_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p]),
    "rans4x16_hip_compress_best_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rans4x16_hip_compress_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rans4x16_hip_uncompress_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_uint32, C.c_uint32, C.c_void_p]),
    "rans4x16_hip_compress_dev_sized": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_int, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]),
    "rans4x16_hip_uncompress_dev_sized": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p]),
    "rans4x16_hip_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_long]),
    "rans4x16_hip_get_option": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_long)]),
    "rans4x16_hip_option_name": (C.c_char_p, [C.c_int]),
    "rans4x16_hip_workspace_bytes": (C.c_size_t, [C.c_void_p]),
    "rans4x16_hip_timing": (None, [C.c_void_p, C.c_int]),
    "rans4x16_hip_timing_read": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_int]),
    "rans4x16_hip_route_read": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_long), C.c_int, C.c_int]),
    "rans4x16_hip_version": (C.c_char_p, []),
    "rans4x16_hip_set_dev_stripe_planes": (C.c_int, [C.c_void_p, C.c_int, C.c_uint]),
    "rans4x16_hip_set_dev_stripe_encode": (C.c_int, [C.c_void_p, C.c_int]),
    "rans4x16_hip_compress_best_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]),
    # the packed device-resident calls: (ctx, n, d_in, d_in_off, d_in_size, d_out, out_capacity, d_out_off, d_out_size, d_status, ..)
    "rans4x16_hip_compress_packed_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_int, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]),
    "rans4x16_hip_compress_best_packed_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]),
    # best of several methods across codecs (part 2m)
    "rans4x16_hip_compress_best_any_packed_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                           C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                           C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]),
    "rans4x16_hip_best_any_chunk_blocks": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_uint64]),
    "rans4x16_hip_uncompress_any_packed_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "rans4x16_hip_compress_best_any_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rans4x16_hip_uncompress_any_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p]),
    # quality blocks: best across rANS 4x16, arith_dynamic and fqzcomp_qual (part 2n)
    "rans4x16_hip_compress_best_qual_packed_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                                            C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                            C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p]),
    "rans4x16_hip_best_qual_chunk_blocks": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64]),
    "rans4x16_hip_uncompress_qual_packed_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                         C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                         C.c_uint32, C.c_uint32, C.c_void_p]),
    "rans4x16_hip_compress_best_qual_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rans4x16_hip_uncompress_qual_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rans4x16_hip_peek_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rans4x16_hip_uncompress_packed_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    # tok3 column containers (include/rans4x16_hip.h part 2c)
    "rans4x16_hip_tok3_scan": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "rans4x16_hip_tok3_scan_any": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                                            C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                            C.POINTER(C.c_int)]),
    "rans4x16_hip_set_tok3_arith": (C.c_int, [C.c_void_p, C.c_int]),
    "rans4x16_hip_tok3_pack_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32,
                                            C.c_uint64, C.c_void_p]),
    "rans4x16_hip_tok3_unpack_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                              C.c_uint32, C.c_void_p]),
    # tok3 name decoding (include/rans4x16_hip.h part 2d)
    "rans4x16_hip_tok3_names_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                             C.c_uint32, C.c_uint32, C.c_void_p]),
    "rans4x16_hip_tok3_decode_names_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                                    C.c_void_p]),
    "rans4x16_hip_device_clock_khz": (C.c_int, [C.c_void_p]),
    "rans4x16_hip_residency": (C.c_int, [C.c_void_p, C.c_int, C.c_uint, C.c_int, C.c_uint, C.POINTER(C.c_int),
                                        C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rans4x16_hip_partition": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "rans4x16_hip_cpulist_parse": (C.c_int, [C.c_char_p, C.c_void_p, C.c_int]),
    "rans4x16_hip_multi_numa_node": (C.c_int, [C.c_void_p, C.c_int]),
    "rans4x16_hip_multi_create": (C.c_void_p, [C.c_int, C.c_void_p]),
    "rans4x16_hip_multi_destroy": (None, [C.c_void_p]),
    "rans4x16_hip_multi_devices": (C.c_int, [C.c_void_p]),
    "rans4x16_hip_multi_last_error": (C.c_char_p, [C.c_void_p]),
    "rans4x16_hip_compress_batch_multi": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "rans4x16_hip_uncompress_batch_multi": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p]),
    # include/rans4x8_hip.h
    "rans_compress": (C.c_void_p, [_u8p, C.c_uint, C.POINTER(C.c_uint), C.c_int]),
    "rans_uncompress": (C.c_void_p, [_u8p, C.c_uint, C.POINTER(C.c_uint)]),
    "rans4x8_hip_compress_bound": (C.c_uint, [C.c_uint]),
    "rans4x8_hip_compress_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "rans4x8_hip_uncompress_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
    "rans4x8_hip_compress_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rans4x8_hip_uncompress_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # tok3 name encoding (include/rans4x16_hip.h part 2e)
    "rans4x16_hip_tok3_tokenise_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                                C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p]),
    "rans4x16_hip_tok3_encode_names_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                    C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p]),
    # tok3 names with host buffers (include/rans4x16_hip.h part 2f)
    "rans4x16_hip_tok3_level_methods": (C.c_int, [C.c_int, C.POINTER(C.c_int)]),
    "rans4x16_hip_tok3_encode_names": (C.c_void_p, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                                   C.POINTER(C.c_int)]),
    "rans4x16_hip_tok3_decode_names": (C.c_void_p, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    "rans4x16_hip_tok3_arith_encode_names": (C.c_void_p, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int),
                                                         C.POINTER(C.c_int)]),
    "rans4x16_hip_tok3_arith_decode_names": (C.c_void_p, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    "rans4x16_hip_thread_ctx": (C.c_void_p, []),
    "rans4x16_hip_tok3_encode_names_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rans4x16_hip_tok3_decode_names_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_void_p]),
    "rans4x16_hip_set_names_chunk_blocks": (C.c_int, [C.c_void_p, C.c_int]),
    # arith_dynamic decoding (include/rans4x16_hip.h part 2g)
    "rans4x16_hip_arith_uncompress_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p]),
    "rans4x16_hip_arith_peek_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rans4x16_hip_arith_uncompress_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p]),
    "rans4x16_hip_arith_uncompress_to": (C.c_void_p, [C.c_void_p, C.c_uint, C.c_void_p, C.POINTER(C.c_uint)]),
    "rans4x16_hip_arith_uncompress": (C.c_void_p, [C.c_void_p, C.c_uint, C.POINTER(C.c_uint)]),
    # arith_dynamic encoding (include/rans4x16_hip.h part 2h)
    "rans4x16_hip_arith_compress_bound": (C.c_uint, [C.c_uint, C.c_int]),
    "rans4x16_hip_arith_compress_cap": (C.c_uint, [C.c_uint, C.c_int]),
    "rans4x16_hip_arith_compress_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_int, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]),
    "rans4x16_hip_arith_compress_best_packed_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                             C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                             C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64,
                                                             C.c_void_p]),
    "rans4x16_hip_arith_best_chunk_blocks": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_uint64]),
    "rans4x16_hip_arith_compress_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "rans4x16_hip_arith_compress_to": (C.c_void_p, [C.c_void_p, C.c_uint, C.c_void_p, C.POINTER(C.c_uint), C.c_int]),
    "rans4x16_hip_arith_compress": (C.c_void_p, [C.c_void_p, C.c_uint, C.POINTER(C.c_uint), C.c_int]),
    # fqzcomp_qual decoding (include/rans4x16_hip.h part 2i)
    "rans4x16_hip_fqz_scan": (C.c_int, [C.c_void_p, C.c_uint, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                       C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "rans4x16_hip_set_fqz_limits": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "rans4x16_hip_fqz_uncompress_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p]),
    "rans4x16_hip_fqz_peek_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rans4x16_hip_fqz_uncompress_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rans4x16_hip_fqz_decompress": (C.c_void_p, [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p, C.c_int]),
    # fqzcomp_qual encoding (include/rans4x16_hip.h part 2j)
    "rans4x16_hip_fqz_pick_parameters": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                  C.c_void_p, C.c_uint, C.POINTER(C.c_uint)]),
    "rans4x16_hip_fqz_compress_cap": (C.c_uint, [C.c_uint, C.c_uint, C.c_uint]),
    "rans4x16_hip_fqz_compress_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "rans4x16_hip_fqz_compress_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rans4x16_hip_fqz_compress": (C.c_void_p, [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_int, C.c_void_p]),
    # fqzcomp_qual encoding: the parameter choice on the device (include/rans4x16_hip.h part 2k)
    "rans4x16_hip_fqz_pick_cap": (C.c_uint, []),
    "rans4x16_hip_set_fqz_pick": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "rans4x16_hip_fqz_pick_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_uint32, C.c_uint32, C.c_void_p]),
    "rans4x16_hip_fqz_compress_pick_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_uint32, C.c_uint32, C.c_void_p]),
    # fqzcomp_qual encoding: best of several strategies (include/rans4x16_hip.h part 2l)
    "rans4x16_hip_fqz_compress_best_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_uint32, C.c_uint32, C.c_void_p]),
    "rans4x16_hip_fqz_compress_best_packed_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                                            C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                            C.c_uint32, C.c_uint32, C.c_void_p]),
    "rans4x16_hip_fqz_best_chunk_blocks": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_uint32]),
    "rans4x16_hip_fqz_compress_best_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # rANS 4x8's packed and best-of-two device-resident calls (include/rans4x8_hip.h part 2a)
    "rans4x8_hip_compress_packed_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rans4x8_hip_compress_best_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rans4x8_hip_compress_best_packed_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rans4x8_hip_peek_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rans4x8_hip_uncompress_packed_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_uint32, C.c_uint32, C.c_void_p]),
}


class LibraryNotBuilt(RuntimeError):
    pass


_lib = None


def load():
    """Load the HIP library.  Raises LibraryNotBuilt if it is missing — the product path never
    substitutes another implementation."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LibraryNotBuilt(
                f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C htscodecs_amd/csrc` (needs hipcc)")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)          # AttributeError here = ABI drift, fail loudly
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib

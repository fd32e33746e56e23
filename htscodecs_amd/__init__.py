"""htscodecs_amd — MI355X (gfx950) implementation of the CRAM 3.1 rANS 4x16 codec.

The product is the C-ABI shared library ``librans4x16_hip.so`` (see include/rans4x16_hip.h);
this package is the thin Python mirror of that interface used by the tests and the benchmark:

* :mod:`htscodecs_amd.lib`  — ctypes binding of every exported symbol (fails loudly if the
  library has not been built; there is no Python or CPU implementation to fall back to);
* :mod:`htscodecs_amd.codec` — the reference's five functions on ``bytes`` plus batch calls on
  device-resident torch tensors.
"""
from .lib import load, LibraryNotBuilt, STATUS_NAMES  # noqa: F401
from .codec import (  # noqa: F401
    rans_compress_bound_4x16, rans_compress_4x16, rans_uncompress_4x16,
    compress_batch, compress_best_batch, uncompress_batch, DeviceCodec, MultiCodec,
    rans_compress, rans_uncompress, compress_batch_4x8, uncompress_batch_4x8,
    tok3_level_methods, tok3_encode_names_batch, tok3_decode_names_batch, encode_names, decode_names,
    tok3_scan_any, set_tok3_arith, TOK3_ARITH_DECODE, TOK3_ARITH_ENCODE,
    arith_uncompress, arith_uncompress_batch,
    arith_compress, arith_compress_batch, arith_compress_bound, arith_compress_cap,
    fqz_scan, fqz_decompress, fqz_uncompress_batch,
    fqz_pick_parameters, fqz_compress, fqz_compress_batch, fqz_compress_best_batch, fqz_compress_cap, fqz_pick_cap,
    compress_best_any_batch, uncompress_any_batch, compress_best_qual_batch, uncompress_qual_batch, CODEC_RANS4X16, CODEC_ARITH, CODEC_MASK, CODEC_FQZ,
)

__all__ = [
    "load", "LibraryNotBuilt", "STATUS_NAMES",
    "rans_compress_bound_4x16", "rans_compress_4x16", "rans_uncompress_4x16",
    "compress_batch", "compress_best_batch", "uncompress_batch", "DeviceCodec", "MultiCodec",
    "rans_compress", "rans_uncompress", "compress_batch_4x8", "uncompress_batch_4x8",
    "tok3_level_methods", "tok3_encode_names_batch", "tok3_decode_names_batch", "encode_names", "decode_names",
    "tok3_scan_any", "set_tok3_arith", "TOK3_ARITH_DECODE", "TOK3_ARITH_ENCODE",
    "arith_uncompress", "arith_uncompress_batch",
    "arith_compress", "arith_compress_batch", "arith_compress_bound", "arith_compress_cap",
    "fqz_scan", "fqz_decompress", "fqz_uncompress_batch",
    "fqz_pick_parameters", "fqz_compress", "fqz_compress_batch", "fqz_compress_best_batch", "fqz_compress_cap", "fqz_pick_cap",
    "compress_best_any_batch", "uncompress_any_batch", "compress_best_qual_batch", "uncompress_qual_batch",
    "CODEC_RANS4X16", "CODEC_ARITH", "CODEC_MASK", "CODEC_FQZ",
]

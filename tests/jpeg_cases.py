"""The inputs of the device JPEG encoder's tests beyond the cases of tests/jpeg_oracle.py: the sizes at the launchers' edges, read off
the constants of include/wct_hip_jpeg.h, and the committed seed whose padded last byte is FF.  tests/test_jpeg_cpu.py checks that each
case is on the side of its edge that it claims; tests/test_jpeg_gpu.py runs them."""
from wct_hip import lib as _lib

# a 16 x 16 noise image (jpeg_oracle.make_image) whose bit count is no multiple of 8 and whose last byte, padded with ones, is FF
FF_TAIL_SEED = 15


def num_blocks(H, W):
    return 6 * ((H + 15) // 16) * ((W + 15) // 16)


# (name, H, W, quantity, relation, constant): `quantity` of the noise image H x W at quality 75 is `relation` the constant.  Every size
# has a ragged right and a ragged bottom MCU.
#   mcus_per_row     MCUs in an MCU row             against WCT_JPEG_SEG_MCUS (the blocks kernel's workgroup)
#   blocks           6 MH MW                        against WCT_JPEG_PACK_SPAN, WCT_JPEG_SCAN_TILE and SCAN_TILE x SCAN_CHUNK
#   stream_bytes     the padded, unstuffed stream   against WCT_JPEG_STUFF_CHUNK and STUFF_CHUNK x SCAN_CHUNK
EDGES = [
    ("seg_below", 21, 101, "mcus_per_row", "<", _lib.JPEG_SEG_MCUS),
    ("seg_above", 21, 131, "mcus_per_row", ">", _lib.JPEG_SEG_MCUS),
    ("span_below", 27, 70, "blocks", "<", _lib.JPEG_PACK_SPAN),
    ("span_above", 9, 170, "blocks", ">", _lib.JPEG_PACK_SPAN),
    ("tile_below", 89, 101, "blocks", "<", _lib.JPEG_SCAN_TILE),
    ("tile_above", 13, 679, "blocks", ">", _lib.JPEG_SCAN_TILE),
    ("stuff_below", 39, 35, "stream_bytes", "<", _lib.JPEG_STUFF_CHUNK),
    ("stuff_above", 37, 40, "stream_bytes", ">=", _lib.JPEG_STUFF_CHUNK),
    # more than one step of both one-workgroup scans: over SCAN_CHUNK tiles of blocks, and over SCAN_CHUNK chunks of stream
    ("two_scan_steps", 1670, 1675, "blocks", ">", _lib.JPEG_SCAN_TILE * _lib.JPEG_SCAN_CHUNK),
]


def holds(value, relation, constant):
    return {"<": value < constant, ">": value > constant, ">=": value >= constant}[relation]

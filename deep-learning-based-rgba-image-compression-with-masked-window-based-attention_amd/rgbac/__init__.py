"""rgbac -- MI355X-native hot path of the learned RGBA codec (masked window attention).

Drop-in mirrors of the reference modules live in ``rgbac.models`` and
``rgbac.layers``; the compute is librgbac_hip.so (C ABI: include/rgbac.h)."""
from . import _lib  # noqa: F401
from .indexexact import (decode_index_planes, encode_index_planes,  # noqa: F401
                         parse_index_planes)
from .rgbalossless import (decode_rgba_lossless, encode_rgba_lossless,  # noqa: F401
                           encode_rgba_lossless_host, parse_rgba_lossless)
from .rgbanear import (decode_rgba_near, encode_rgba_near, encode_rgba_near_host,  # noqa: F401
                       parse_rgba_near)

__version__ = "0.1.0"

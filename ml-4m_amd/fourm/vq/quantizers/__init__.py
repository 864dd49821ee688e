from .quantize_lucid import VectorQuantize as VectorQuantizerLucid
from .quantize_memcodes import Memcodes

from fourm import _upstream as _up

_up.extend_path(__name__, __path__)

from .bottom_up_decoder import BottomUpHeatMapAEDecoder, resize_bilinear  # noqa: F401
from .decoder import Decoder  # noqa: F401
from .top_down_decoder import TopDownHeatMapDecoder  # noqa: F401

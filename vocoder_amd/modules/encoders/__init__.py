from .convnext import ConvNeXtEncoder  # noqa: F401
from .hubert import HubertEncoder  # noqa: F401
from .mms import MMSEncoder  # noqa: F401
from .posterior_encoder import PosteriorEncoder, PosteriorPool, PosteriorStream  # noqa: F401

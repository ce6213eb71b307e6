from .mpd import DiscriminatorP, MultiPeriodDiscriminator
from .mrd import DiscriminatorR, MultiResolutionDiscriminator

__all__ = ["DiscriminatorP", "MultiPeriodDiscriminator", "DiscriminatorR", "MultiResolutionDiscriminator"]

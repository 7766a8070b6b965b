from .logit import LogitICARGibbs, LogitRSRGibbs
from .probit import ProbitRSRGibbs

__all__ = ('LogitICARGibbs', 'LogitRSRGibbs', 'ProbitRSRGibbs')

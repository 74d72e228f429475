from .allnorm_uncentered import *  # noqa: F401,F403
from .batchnorm_uncentered import *  # noqa: F401,F403
from .groupnorm_uncentered import *  # noqa: F401,F403
from .posnorm_uncentered import *  # noqa: F401,F403

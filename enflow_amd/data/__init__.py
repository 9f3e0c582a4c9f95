from .base import Data, Edges, DataLoader  # noqa: F401
from .edge_list import EdgeList  # noqa: F401

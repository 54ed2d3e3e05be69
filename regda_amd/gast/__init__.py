from .triple import TripletLoss  # noqa: F401

from . import all_neighbors, ball_cover, brute_force, cagra, epsilon_neighborhood, hnsw, ivf_flat, ivf_pq, ivf_rabitq, ivf_sq, mg, scann, sparse_brute_force, tiered_index, vamana  # noqa: F401
from .refine import refine  # noqa: F401

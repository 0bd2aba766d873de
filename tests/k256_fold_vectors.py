"""Inputs that drive every column of the k256 products to its maximum (fe_k256.hpp: mul, mul_add2, mul_add_sqr): the k256 raw
section of tests/field_edge_vectors.py, under the name its first users import."""
from field_edge_vectors import EDGES, P, TOP, WORDS, extreme, high_ones_pair, pairs, quads, to_bytes  # noqa: F401

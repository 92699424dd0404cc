"""CPU checks of the device marching cubes (hn_mcubes.hip, honerf_amd.mesh): its C ABI, a numpy restatement of the mesher that
the GPU tests (tests/test_mesh.py) compare against exactly, the restatement's tables case by case, its surface on an analytic
sphere, and the PLY export (honerf_amd.harness.write_ply / read_ply)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the restatement: the classic 256-case tables (Lorensen / Bourke numbering) ------------------------------------------------
# corner c at (x, y, z); edge e joins EDGE_CORNERS[e]; a corner is inside (its bit set in the case) when value < threshold
CORNERS = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)])
EDGE_CORNERS = [(0, 1), (1, 2), (3, 2), (0, 3), (4, 5), (5, 6), (7, 6), (4, 7), (0, 4), (1, 5), (2, 6), (3, 7)]
# an edge's owner: its first corner (offset from the cell origin) and its axis
EDGE_OWNER = [(tuple(CORNERS[a]), int(np.argmax(CORNERS[b] - CORNERS[a]))) for a, b in EDGE_CORNERS]
EDGE_TABLE = [
    0x000, 0x109, 0x203, 0x30a, 0x406, 0x50f, 0x605, 0x70c, 0x80c, 0x905, 0xa0f, 0xb06, 0xc0a, 0xd03, 0xe09, 0xf00,
    0x190, 0x099, 0x393, 0x29a, 0x596, 0x49f, 0x795, 0x69c, 0x99c, 0x895, 0xb9f, 0xa96, 0xd9a, 0xc93, 0xf99, 0xe90,
    0x230, 0x339, 0x033, 0x13a, 0x636, 0x73f, 0x435, 0x53c, 0xa3c, 0xb35, 0x83f, 0x936, 0xe3a, 0xf33, 0xc39, 0xd30,
    0x3a0, 0x2a9, 0x1a3, 0x0aa, 0x7a6, 0x6af, 0x5a5, 0x4ac, 0xbac, 0xaa5, 0x9af, 0x8a6, 0xfaa, 0xea3, 0xda9, 0xca0,
    0x460, 0x569, 0x663, 0x76a, 0x066, 0x16f, 0x265, 0x36c, 0xc6c, 0xd65, 0xe6f, 0xf66, 0x86a, 0x963, 0xa69, 0xb60,
    0x5f0, 0x4f9, 0x7f3, 0x6fa, 0x1f6, 0x0ff, 0x3f5, 0x2fc, 0xdfc, 0xcf5, 0xfff, 0xef6, 0x9fa, 0x8f3, 0xbf9, 0xaf0,
    0x650, 0x759, 0x453, 0x55a, 0x256, 0x35f, 0x055, 0x15c, 0xe5c, 0xf55, 0xc5f, 0xd56, 0xa5a, 0xb53, 0x859, 0x950,
    0x7c0, 0x6c9, 0x5c3, 0x4ca, 0x3c6, 0x2cf, 0x1c5, 0x0cc, 0xfcc, 0xec5, 0xdcf, 0xcc6, 0xbca, 0xac3, 0x9c9, 0x8c0,
    0x8c0, 0x9c9, 0xac3, 0xbca, 0xcc6, 0xdcf, 0xec5, 0xfcc, 0x0cc, 0x1c5, 0x2cf, 0x3c6, 0x4ca, 0x5c3, 0x6c9, 0x7c0,
    0x950, 0x859, 0xb53, 0xa5a, 0xd56, 0xc5f, 0xf55, 0xe5c, 0x15c, 0x055, 0x35f, 0x256, 0x55a, 0x453, 0x759, 0x650,
    0xaf0, 0xbf9, 0x8f3, 0x9fa, 0xef6, 0xfff, 0xcf5, 0xdfc, 0x2fc, 0x3f5, 0x0ff, 0x1f6, 0x6fa, 0x7f3, 0x4f9, 0x5f0,
    0xb60, 0xa69, 0x963, 0x86a, 0xf66, 0xe6f, 0xd65, 0xc6c, 0x36c, 0x265, 0x16f, 0x066, 0x76a, 0x663, 0x569, 0x460,
    0xca0, 0xda9, 0xea3, 0xfaa, 0x8a6, 0x9af, 0xaa5, 0xbac, 0x4ac, 0x5a5, 0x6af, 0x7a6, 0x0aa, 0x1a3, 0x2a9, 0x3a0,
    0xd30, 0xc39, 0xf33, 0xe3a, 0x936, 0x83f, 0xb35, 0xa3c, 0x53c, 0x435, 0x73f, 0x636, 0x13a, 0x033, 0x339, 0x230,
    0xe90, 0xf99, 0xc93, 0xd9a, 0xa96, 0xb9f, 0x895, 0x99c, 0x69c, 0x795, 0x49f, 0x596, 0x29a, 0x393, 0x099, 0x190,
    0xf00, 0xe09, 0xd03, 0xc0a, 0xb06, 0xa0f, 0x905, 0x80c, 0x70c, 0x605, 0x50f, 0x406, 0x30a, 0x203, 0x109, 0x000,
]
TRI_TABLE = [
    (),
    (0, 8, 3),
    (0, 1, 9),
    (1, 8, 3, 9, 8, 1),
    (1, 2, 10),
    (0, 8, 3, 1, 2, 10),
    (9, 2, 10, 0, 2, 9),
    (2, 8, 3, 2, 10, 8, 10, 9, 8),
    (3, 11, 2),
    (0, 11, 2, 8, 11, 0),
    (1, 9, 0, 2, 3, 11),
    (1, 11, 2, 1, 9, 11, 9, 8, 11),
    (3, 10, 1, 11, 10, 3),
    (0, 10, 1, 0, 8, 10, 8, 11, 10),
    (3, 9, 0, 3, 11, 9, 11, 10, 9),
    (9, 8, 10, 10, 8, 11),
    (4, 7, 8),
    (4, 3, 0, 7, 3, 4),
    (0, 1, 9, 8, 4, 7),
    (4, 1, 9, 4, 7, 1, 7, 3, 1),
    (1, 2, 10, 8, 4, 7),
    (3, 4, 7, 3, 0, 4, 1, 2, 10),
    (9, 2, 10, 9, 0, 2, 8, 4, 7),
    (2, 10, 9, 2, 9, 7, 2, 7, 3, 7, 9, 4),
    (8, 4, 7, 3, 11, 2),
    (11, 4, 7, 11, 2, 4, 2, 0, 4),
    (9, 0, 1, 8, 4, 7, 2, 3, 11),
    (4, 7, 11, 9, 4, 11, 9, 11, 2, 9, 2, 1),
    (3, 10, 1, 3, 11, 10, 7, 8, 4),
    (1, 11, 10, 1, 4, 11, 1, 0, 4, 7, 11, 4),
    (4, 7, 8, 9, 0, 11, 9, 11, 10, 11, 0, 3),
    (4, 7, 11, 4, 11, 9, 9, 11, 10),
    (9, 5, 4),
    (9, 5, 4, 0, 8, 3),
    (0, 5, 4, 1, 5, 0),
    (8, 5, 4, 8, 3, 5, 3, 1, 5),
    (1, 2, 10, 9, 5, 4),
    (3, 0, 8, 1, 2, 10, 4, 9, 5),
    (5, 2, 10, 5, 4, 2, 4, 0, 2),
    (2, 10, 5, 3, 2, 5, 3, 5, 4, 3, 4, 8),
    (9, 5, 4, 2, 3, 11),
    (0, 11, 2, 0, 8, 11, 4, 9, 5),
    (0, 5, 4, 0, 1, 5, 2, 3, 11),
    (2, 1, 5, 2, 5, 8, 2, 8, 11, 4, 8, 5),
    (10, 3, 11, 10, 1, 3, 9, 5, 4),
    (4, 9, 5, 0, 8, 1, 8, 10, 1, 8, 11, 10),
    (5, 4, 0, 5, 0, 11, 5, 11, 10, 11, 0, 3),
    (5, 4, 8, 5, 8, 10, 10, 8, 11),
    (9, 7, 8, 5, 7, 9),
    (9, 3, 0, 9, 5, 3, 5, 7, 3),
    (0, 7, 8, 0, 1, 7, 1, 5, 7),
    (1, 5, 3, 3, 5, 7),
    (9, 7, 8, 9, 5, 7, 10, 1, 2),
    (10, 1, 2, 9, 5, 0, 5, 3, 0, 5, 7, 3),
    (8, 0, 2, 8, 2, 5, 8, 5, 7, 10, 5, 2),
    (2, 10, 5, 2, 5, 3, 3, 5, 7),
    (7, 9, 5, 7, 8, 9, 3, 11, 2),
    (9, 5, 7, 9, 7, 2, 9, 2, 0, 2, 7, 11),
    (2, 3, 11, 0, 1, 8, 1, 7, 8, 1, 5, 7),
    (11, 2, 1, 11, 1, 7, 7, 1, 5),
    (9, 5, 8, 8, 5, 7, 10, 1, 3, 10, 3, 11),
    (5, 7, 0, 5, 0, 9, 7, 11, 0, 1, 0, 10, 11, 10, 0),
    (11, 10, 0, 11, 0, 3, 10, 5, 0, 8, 0, 7, 5, 7, 0),
    (11, 10, 5, 7, 11, 5),
    (10, 6, 5),
    (0, 8, 3, 5, 10, 6),
    (9, 0, 1, 5, 10, 6),
    (1, 8, 3, 1, 9, 8, 5, 10, 6),
    (1, 6, 5, 2, 6, 1),
    (1, 6, 5, 1, 2, 6, 3, 0, 8),
    (9, 6, 5, 9, 0, 6, 0, 2, 6),
    (5, 9, 8, 5, 8, 2, 5, 2, 6, 3, 2, 8),
    (2, 3, 11, 10, 6, 5),
    (11, 0, 8, 11, 2, 0, 10, 6, 5),
    (0, 1, 9, 2, 3, 11, 5, 10, 6),
    (5, 10, 6, 1, 9, 2, 9, 11, 2, 9, 8, 11),
    (6, 3, 11, 6, 5, 3, 5, 1, 3),
    (0, 8, 11, 0, 11, 5, 0, 5, 1, 5, 11, 6),
    (3, 11, 6, 0, 3, 6, 0, 6, 5, 0, 5, 9),
    (6, 5, 9, 6, 9, 11, 11, 9, 8),
    (5, 10, 6, 4, 7, 8),
    (4, 3, 0, 4, 7, 3, 6, 5, 10),
    (1, 9, 0, 5, 10, 6, 8, 4, 7),
    (10, 6, 5, 1, 9, 7, 1, 7, 3, 7, 9, 4),
    (6, 1, 2, 6, 5, 1, 4, 7, 8),
    (1, 2, 5, 5, 2, 6, 3, 0, 4, 3, 4, 7),
    (8, 4, 7, 9, 0, 5, 0, 6, 5, 0, 2, 6),
    (7, 3, 9, 7, 9, 4, 3, 2, 9, 5, 9, 6, 2, 6, 9),
    (3, 11, 2, 7, 8, 4, 10, 6, 5),
    (5, 10, 6, 4, 7, 2, 4, 2, 0, 2, 7, 11),
    (0, 1, 9, 4, 7, 8, 2, 3, 11, 5, 10, 6),
    (9, 2, 1, 9, 11, 2, 9, 4, 11, 7, 11, 4, 5, 10, 6),
    (8, 4, 7, 3, 11, 5, 3, 5, 1, 5, 11, 6),
    (5, 1, 11, 5, 11, 6, 1, 0, 11, 7, 11, 4, 0, 4, 11),
    (0, 5, 9, 0, 6, 5, 0, 3, 6, 11, 6, 3, 8, 4, 7),
    (6, 5, 9, 6, 9, 11, 4, 7, 9, 7, 11, 9),
    (10, 4, 9, 6, 4, 10),
    (4, 10, 6, 4, 9, 10, 0, 8, 3),
    (10, 0, 1, 10, 6, 0, 6, 4, 0),
    (8, 3, 1, 8, 1, 6, 8, 6, 4, 6, 1, 10),
    (1, 4, 9, 1, 2, 4, 2, 6, 4),
    (3, 0, 8, 1, 2, 9, 2, 4, 9, 2, 6, 4),
    (0, 2, 4, 4, 2, 6),
    (8, 3, 2, 8, 2, 4, 4, 2, 6),
    (10, 4, 9, 10, 6, 4, 11, 2, 3),
    (0, 8, 2, 2, 8, 11, 4, 9, 10, 4, 10, 6),
    (3, 11, 2, 0, 1, 6, 0, 6, 4, 6, 1, 10),
    (6, 4, 1, 6, 1, 10, 4, 8, 1, 2, 1, 11, 8, 11, 1),
    (9, 6, 4, 9, 3, 6, 9, 1, 3, 11, 6, 3),
    (8, 11, 1, 8, 1, 0, 11, 6, 1, 9, 1, 4, 6, 4, 1),
    (3, 11, 6, 3, 6, 0, 0, 6, 4),
    (6, 4, 8, 11, 6, 8),
    (7, 10, 6, 7, 8, 10, 8, 9, 10),
    (0, 7, 3, 0, 10, 7, 0, 9, 10, 6, 7, 10),
    (10, 6, 7, 1, 10, 7, 1, 7, 8, 1, 8, 0),
    (10, 6, 7, 10, 7, 1, 1, 7, 3),
    (1, 2, 6, 1, 6, 8, 1, 8, 9, 8, 6, 7),
    (2, 6, 9, 2, 9, 1, 6, 7, 9, 0, 9, 3, 7, 3, 9),
    (7, 8, 0, 7, 0, 6, 6, 0, 2),
    (7, 3, 2, 6, 7, 2),
    (2, 3, 11, 10, 6, 8, 10, 8, 9, 8, 6, 7),
    (2, 0, 7, 2, 7, 11, 0, 9, 7, 6, 7, 10, 9, 10, 7),
    (1, 8, 0, 1, 7, 8, 1, 10, 7, 6, 7, 10, 2, 3, 11),
    (11, 2, 1, 11, 1, 7, 10, 6, 1, 6, 7, 1),
    (8, 9, 6, 8, 6, 7, 9, 1, 6, 11, 6, 3, 1, 3, 6),
    (0, 9, 1, 11, 6, 7),
    (7, 8, 0, 7, 0, 6, 3, 11, 0, 11, 6, 0),
    (7, 11, 6),
    (7, 6, 11),
    (3, 0, 8, 11, 7, 6),
    (0, 1, 9, 11, 7, 6),
    (8, 1, 9, 8, 3, 1, 11, 7, 6),
    (10, 1, 2, 6, 11, 7),
    (1, 2, 10, 3, 0, 8, 6, 11, 7),
    (2, 9, 0, 2, 10, 9, 6, 11, 7),
    (6, 11, 7, 2, 10, 3, 10, 8, 3, 10, 9, 8),
    (7, 2, 3, 6, 2, 7),
    (7, 0, 8, 7, 6, 0, 6, 2, 0),
    (2, 7, 6, 2, 3, 7, 0, 1, 9),
    (1, 6, 2, 1, 8, 6, 1, 9, 8, 8, 7, 6),
    (10, 7, 6, 10, 1, 7, 1, 3, 7),
    (10, 7, 6, 1, 7, 10, 1, 8, 7, 1, 0, 8),
    (0, 3, 7, 0, 7, 10, 0, 10, 9, 6, 10, 7),
    (7, 6, 10, 7, 10, 8, 8, 10, 9),
    (6, 8, 4, 11, 8, 6),
    (3, 6, 11, 3, 0, 6, 0, 4, 6),
    (8, 6, 11, 8, 4, 6, 9, 0, 1),
    (9, 4, 6, 9, 6, 3, 9, 3, 1, 11, 3, 6),
    (6, 8, 4, 6, 11, 8, 2, 10, 1),
    (1, 2, 10, 3, 0, 11, 0, 6, 11, 0, 4, 6),
    (4, 11, 8, 4, 6, 11, 0, 2, 9, 2, 10, 9),
    (10, 9, 3, 10, 3, 2, 9, 4, 3, 11, 3, 6, 4, 6, 3),
    (8, 2, 3, 8, 4, 2, 4, 6, 2),
    (0, 4, 2, 4, 6, 2),
    (1, 9, 0, 2, 3, 4, 2, 4, 6, 4, 3, 8),
    (1, 9, 4, 1, 4, 2, 2, 4, 6),
    (8, 1, 3, 8, 6, 1, 8, 4, 6, 6, 10, 1),
    (10, 1, 0, 10, 0, 6, 6, 0, 4),
    (4, 6, 3, 4, 3, 8, 6, 10, 3, 0, 3, 9, 10, 9, 3),
    (10, 9, 4, 6, 10, 4),
    (4, 9, 5, 7, 6, 11),
    (0, 8, 3, 4, 9, 5, 11, 7, 6),
    (5, 0, 1, 5, 4, 0, 7, 6, 11),
    (11, 7, 6, 8, 3, 4, 3, 5, 4, 3, 1, 5),
    (9, 5, 4, 10, 1, 2, 7, 6, 11),
    (6, 11, 7, 1, 2, 10, 0, 8, 3, 4, 9, 5),
    (7, 6, 11, 5, 4, 10, 4, 2, 10, 4, 0, 2),
    (3, 4, 8, 3, 5, 4, 3, 2, 5, 10, 5, 2, 11, 7, 6),
    (7, 2, 3, 7, 6, 2, 5, 4, 9),
    (9, 5, 4, 0, 8, 6, 0, 6, 2, 6, 8, 7),
    (3, 6, 2, 3, 7, 6, 1, 5, 0, 5, 4, 0),
    (6, 2, 8, 6, 8, 7, 2, 1, 8, 4, 8, 5, 1, 5, 8),
    (9, 5, 4, 10, 1, 6, 1, 7, 6, 1, 3, 7),
    (1, 6, 10, 1, 7, 6, 1, 0, 7, 8, 7, 0, 9, 5, 4),
    (4, 0, 10, 4, 10, 5, 0, 3, 10, 6, 10, 7, 3, 7, 10),
    (7, 6, 10, 7, 10, 8, 5, 4, 10, 4, 8, 10),
    (6, 9, 5, 6, 11, 9, 11, 8, 9),
    (3, 6, 11, 0, 6, 3, 0, 5, 6, 0, 9, 5),
    (0, 11, 8, 0, 5, 11, 0, 1, 5, 5, 6, 11),
    (6, 11, 3, 6, 3, 5, 5, 3, 1),
    (1, 2, 10, 9, 5, 11, 9, 11, 8, 11, 5, 6),
    (0, 11, 3, 0, 6, 11, 0, 9, 6, 5, 6, 9, 1, 2, 10),
    (11, 8, 5, 11, 5, 6, 8, 0, 5, 10, 5, 2, 0, 2, 5),
    (6, 11, 3, 6, 3, 5, 2, 10, 3, 10, 5, 3),
    (5, 8, 9, 5, 2, 8, 5, 6, 2, 3, 8, 2),
    (9, 5, 6, 9, 6, 0, 0, 6, 2),
    (1, 5, 8, 1, 8, 0, 5, 6, 8, 3, 8, 2, 6, 2, 8),
    (1, 5, 6, 2, 1, 6),
    (1, 3, 6, 1, 6, 10, 3, 8, 6, 5, 6, 9, 8, 9, 6),
    (10, 1, 0, 10, 0, 6, 9, 5, 0, 5, 6, 0),
    (0, 3, 8, 5, 6, 10),
    (10, 5, 6),
    (11, 5, 10, 7, 5, 11),
    (11, 5, 10, 11, 7, 5, 8, 3, 0),
    (5, 11, 7, 5, 10, 11, 1, 9, 0),
    (10, 7, 5, 10, 11, 7, 9, 8, 1, 8, 3, 1),
    (11, 1, 2, 11, 7, 1, 7, 5, 1),
    (0, 8, 3, 1, 2, 7, 1, 7, 5, 7, 2, 11),
    (9, 7, 5, 9, 2, 7, 9, 0, 2, 2, 11, 7),
    (7, 5, 2, 7, 2, 11, 5, 9, 2, 3, 2, 8, 9, 8, 2),
    (2, 5, 10, 2, 3, 5, 3, 7, 5),
    (8, 2, 0, 8, 5, 2, 8, 7, 5, 10, 2, 5),
    (9, 0, 1, 5, 10, 3, 5, 3, 7, 3, 10, 2),
    (9, 8, 2, 9, 2, 1, 8, 7, 2, 10, 2, 5, 7, 5, 2),
    (1, 3, 5, 3, 7, 5),
    (0, 8, 7, 0, 7, 1, 1, 7, 5),
    (9, 0, 3, 9, 3, 5, 5, 3, 7),
    (9, 8, 7, 5, 9, 7),
    (5, 8, 4, 5, 10, 8, 10, 11, 8),
    (5, 0, 4, 5, 11, 0, 5, 10, 11, 11, 3, 0),
    (0, 1, 9, 8, 4, 10, 8, 10, 11, 10, 4, 5),
    (10, 11, 4, 10, 4, 5, 11, 3, 4, 9, 4, 1, 3, 1, 4),
    (2, 5, 1, 2, 8, 5, 2, 11, 8, 4, 5, 8),
    (0, 4, 11, 0, 11, 3, 4, 5, 11, 2, 11, 1, 5, 1, 11),
    (0, 2, 5, 0, 5, 9, 2, 11, 5, 4, 5, 8, 11, 8, 5),
    (9, 4, 5, 2, 11, 3),
    (2, 5, 10, 3, 5, 2, 3, 4, 5, 3, 8, 4),
    (5, 10, 2, 5, 2, 4, 4, 2, 0),
    (3, 10, 2, 3, 5, 10, 3, 8, 5, 4, 5, 8, 0, 1, 9),
    (5, 10, 2, 5, 2, 4, 1, 9, 2, 9, 4, 2),
    (8, 4, 5, 8, 5, 3, 3, 5, 1),
    (0, 4, 5, 1, 0, 5),
    (8, 4, 5, 8, 5, 3, 9, 0, 5, 0, 3, 5),
    (9, 4, 5),
    (4, 11, 7, 4, 9, 11, 9, 10, 11),
    (0, 8, 3, 4, 9, 7, 9, 11, 7, 9, 10, 11),
    (1, 10, 11, 1, 11, 4, 1, 4, 0, 7, 4, 11),
    (3, 1, 4, 3, 4, 8, 1, 10, 4, 7, 4, 11, 10, 11, 4),
    (4, 11, 7, 9, 11, 4, 9, 2, 11, 9, 1, 2),
    (9, 7, 4, 9, 11, 7, 9, 1, 11, 2, 11, 1, 0, 8, 3),
    (11, 7, 4, 11, 4, 2, 2, 4, 0),
    (11, 7, 4, 11, 4, 2, 8, 3, 4, 3, 2, 4),
    (2, 9, 10, 2, 7, 9, 2, 3, 7, 7, 4, 9),
    (9, 10, 7, 9, 7, 4, 10, 2, 7, 8, 7, 0, 2, 0, 7),
    (3, 7, 10, 3, 10, 2, 7, 4, 10, 1, 10, 0, 4, 0, 10),
    (1, 10, 2, 8, 7, 4),
    (4, 9, 1, 4, 1, 7, 7, 1, 3),
    (4, 9, 1, 4, 1, 7, 0, 8, 1, 8, 7, 1),
    (4, 0, 3, 7, 4, 3),
    (4, 8, 7),
    (9, 10, 8, 10, 11, 8),
    (3, 0, 9, 3, 9, 11, 11, 9, 10),
    (0, 1, 10, 0, 10, 8, 8, 10, 11),
    (3, 1, 10, 11, 3, 10),
    (1, 2, 11, 1, 11, 9, 9, 11, 8),
    (3, 0, 9, 3, 9, 11, 1, 2, 9, 2, 11, 9),
    (0, 2, 11, 8, 0, 11),
    (3, 2, 11),
    (2, 3, 8, 2, 8, 10, 10, 8, 9),
    (9, 10, 2, 0, 9, 2),
    (2, 3, 8, 2, 8, 10, 0, 1, 8, 1, 10, 8),
    (1, 10, 2),
    (1, 3, 8, 9, 1, 8),
    (0, 9, 1),
    (0, 3, 8),
    (),
]


def case_of_corners(inside8):
    return sum(int(b) << c for c, b in enumerate(inside8))


def np_marching_cubes(vol, threshold=0.0):
    """The mesher in numpy, with the device's conventions: vertices float32 [V,3] in index space (one per crossing grid edge, ordered
    by the lower grid point and then axis), triangles int64 [T,3] (by cell, then table order, each reversed so that it faces
    increasing value).  Same fp32 operations as the kernel: t = (thr - v0) / (v1 - v0), coordinate = index + t."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    nx, ny, nz = vol.shape
    thr = np.float32(threshold)
    inside = vol < thr
    cross = np.zeros(vol.shape + (3,), dtype=bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    vid = (np.cumsum(cross.reshape(-1)) - 1).reshape(cross.shape)
    p, a = np.nonzero(cross.reshape(-1, 3))
    idx = np.stack(np.unravel_index(p, vol.shape), -1)
    v0 = vol.reshape(-1)[p]
    step = np.array([ny * nz, nz, 1])[a]
    v1 = vol.reshape(-1)[p + step]
    t = (thr - v0) / (v1 - v0)
    verts = idx.astype(np.float32)
    verts[np.arange(len(p)), a] += t
    # cells
    case = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for c, (dx, dy, dz) in enumerate(CORNERS):
        case |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    ntab = np.array([len(r) // 3 for r in TRI_TABLE])
    tt = np.full((256, 15), -1, dtype=np.int64)
    for c, r in enumerate(TRI_TABLE):
        tt[c, :len(r)] = r
    cells = np.stack(np.nonzero(ntab[case] > 0), -1)
    cc = case[tuple(cells.T)]
    cnt = ntab[cc]
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    tris = np.empty((int(cnt.sum()), 3), dtype=np.int64)
    for s in range(5):
        sel = cnt > s
        for u in range(3):
            e = tt[cc[sel], 3 * s + u]
            own = np.array([EDGE_OWNER[k][0] for k in range(12)])[e]
            ax = np.array([EDGE_OWNER[k][1] for k in range(12)])[e]
            o = cells[sel] + own
            tris[first[sel] + s, 2 - u] = vid[o[:, 0], o[:, 1], o[:, 2], ax]
    return verts, tris


def sphere_volume(res, r=0.3):
    ax = np.linspace(-0.5, 0.5, res, dtype=np.float32)
    x, y, z = np.meshgrid(ax, ax, ax, indexing='ij')
    return (np.sqrt(x * x + y * y + z * z) - np.float32(r)).astype(np.float32)


def torus_volume(res, R=0.3, r=0.1):
    ax = np.linspace(-0.5, 0.5, res, dtype=np.float32)
    x, y, z = np.meshgrid(ax, ax, ax, indexing='ij')
    q = np.sqrt(x * x + y * y) - np.float32(R)
    return (np.sqrt(q * q + z * z) - np.float32(r)).astype(np.float32)


def noise_volume(shape=(23, 19, 17), seed=5):
    return np.random.RandomState(seed).randn(*shape).astype(np.float32)


def cases_present(vol, threshold=0.0):
    inside = np.asarray(vol) < np.float32(threshold)
    nx, ny, nz = inside.shape
    case = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for c, (dx, dy, dz) in enumerate(CORNERS):
        case |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    return set(np.unique(case).tolist())


def edge_stats(tris):
    """(undirected edges used by other than exactly two faces, directed edges used more than once)."""
    d = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]])
    _, dn = np.unique(d, axis=0, return_counts=True)
    _, un = np.unique(np.sort(d, axis=1), axis=0, return_counts=True)
    return int((un != 2).sum()), int((dn != 1).sum())


def euler(verts, tris):
    d = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]])
    E = len(np.unique(np.sort(d, axis=1), axis=0))
    return len(verts) - E + len(tris)


def area_volume(verts, tris):
    v = np.asarray(verts, dtype=np.float64)
    a, b, c = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum()
    vol = np.einsum('ij,ij->i', a, np.cross(b, c)).sum() / 6.0
    return area, vol


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_header_and_library_carry_the_mesher():
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'honerf.h')).read(), flags=re.S)
    names = set(re.findall(r'\b(hn_mcubes[a-z0-9_]*)\s*\(', src))
    assert names == {'hn_mcubes_workspace_bytes', 'hn_mcubes_count', 'hn_mcubes_emit'}, names
    from honerf_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for n in names:
        assert hasattr(cdll, n), n
        assert n in lib.SIGNATURES, n
    L = lib.load()
    assert L.hn_mcubes_workspace_bytes(64, 64, 64) > 64 ** 3 * 5
    assert L.hn_mcubes_workspace_bytes(1, 64, 64) == 0          # dims below 2 are refused
    assert L.hn_mcubes_workspace_bytes(1024, 1024, 1024) == 0   # 3 n >= 2^31: edge ids would overflow int32
    assert L.hn_mcubes_workspace_bytes(2, 2, 2) > 0


def test_mesher_source_has_no_scalar_memory_writes():
    src = open(os.path.join(ROOT, 'ho-nerf_amd', 'csrc', 'hn_mcubes.hip')).read().lower()
    for w in ('s_' + 'store', 's_' + 'buffer', 's_' + 'scratch', 's_' + 'atomic', 's_' + 'dcache'):
        assert w not in src, w


# ---- the tables, case by case ------------------------------------------------------------------------------------------------
def crossing(case):
    return {e for e, (a, b) in enumerate(EDGE_CORNERS) if (case >> a & 1) != (case >> b & 1)}


@pytest.mark.parametrize('case', range(256))
def test_table_case_uses_exactly_its_crossing_edges(case):
    tri = TRI_TABLE[case]
    assert len(tri) % 3 == 0 and len(tri) <= 15
    assert set(tri) == crossing(case)
    assert EDGE_TABLE[case] == sum(1 << e for e in crossing(case))
    assert set(TRI_TABLE[255 - case]) == set(tri)      # the complementary case uses the same edge set
    tris = [tuple(tri[i:i + 3]) for i in range(0, len(tri), 3)]
    assert all(len(set(t)) == 3 for t in tris)


def test_tables_close_up_across_cells():
    """Inside a cell every directed edge of the patch occurs once and the open ones lie on cube faces; across a face, the segments
    the two cells leave there are the same with opposite directions (so a mesh is watertight and consistently oriented)."""
    faces = {'x0': [0, 3, 7, 4], 'x1': [1, 2, 6, 5], 'y0': [0, 1, 5, 4], 'y1': [3, 2, 6, 7], 'z0': [0, 1, 2, 3], 'z1': [4, 5, 6, 7]}
    fedges = {f: {e for e, (a, b) in enumerate(EDGE_CORNERS) if a in c and b in c} for f, c in faces.items()}
    segs = {}
    for case in range(256):
        tri = TRI_TABLE[case]
        d = {}
        for i in range(0, len(tri), 3):
            a, b, c = tri[i:i + 3]
            for uv in ((a, b), (b, c), (c, a)):
                d[uv] = d.get(uv, 0) + 1
        assert max(d.values(), default=1) == 1, case
        open_ = [(u, v) for (u, v) in d if (v, u) not in d]
        for u, v in open_:
            assert any(u in fe and v in fe for fe in fedges.values()), (case, u, v)
        for f, c in faces.items():
            key = (f, tuple(case >> k & 1 for k in c))
            s = frozenset(uv for uv in open_ if uv[0] in fedges[f] and uv[1] in fedges[f])
            assert segs.setdefault(key, s) == s, key
    pairs = {('x1', 'x0'): {1: 3, 5: 7, 9: 8, 10: 11}, ('y1', 'y0'): {2: 0, 6: 4, 11: 8, 10: 9}, ('z1', 'z0'): {4: 0, 5: 1, 6: 2, 7: 3}}
    for (fa, fb), m in pairs.items():
        for bits in range(16):
            k = tuple(bits >> i & 1 for i in range(4))
            assert frozenset((m[v], m[u]) for u, v in segs[(fa, k)]) == segs[(fb, k)], (fa, k)


# ---- the restatement on analytic surfaces ------------------------------------------------------------------------------------
def test_numpy_mesher_sphere_is_watertight_and_outward():
    res = 40
    vol = sphere_volume(res)
    v, t = np_marching_cubes(vol, 0.0)
    assert len(v) > 0 and len(t) > 0
    assert edge_stats(t) == (0, 0)
    assert euler(v, t) == 2
    assert len(np.unique(t)) == len(v)               # every vertex is used
    h = 1.0 / (res - 1)
    area, volume = area_volume(v * h - 0.5, t)
    assert volume > 0                                 # faces point toward increasing value: outward
    assert abs(volume / (4 / 3 * np.pi * 0.3 ** 3) - 1) < 0.03
    assert abs(area / (4 * np.pi * 0.3 ** 2) - 1) < 0.03


def test_numpy_mesher_orders_and_shares_vertices():
    vol = noise_volume((7, 6, 5), seed=1)
    v, t = np_marching_cubes(vol, 0.1)
    inside = vol < np.float32(0.1)
    n_cross = (inside[1:] != inside[:-1]).sum() + (inside[:, 1:] != inside[:, :-1]).sum() + (inside[:, :, 1:] != inside[:, :, :-1]).sum()
    assert len(v) == n_cross
    assert len(np.unique(t)) == len(v)
    # vertices sorted by (owning point, axis): the owner is floor of the coordinates
    own = np.floor(v).astype(np.int64)
    lin = (own[:, 0] * 6 + own[:, 1]) * 5 + own[:, 2]
    assert (np.diff(lin) >= 0).all()


# ---- PLY ---------------------------------------------------------------------------------------------------------------------
def test_ply_round_trip_is_bit_exact(tmp_path):
    from honerf_amd import harness
    v, t = np_marching_cubes(sphere_volume(20), 0.0)
    v = (v * np.float32(0.01) - np.float32(0.1)).astype(np.float32)
    p = str(tmp_path / 'm.ply')
    harness.write_ply(p, v, t)
    v2, t2 = harness.read_ply(p)
    assert v2.dtype == np.float32 and t2.dtype == np.int64
    assert v2.tobytes() == v.tobytes() and np.array_equal(t2, t)
    head = open(p, 'rb').read(200)
    assert head.startswith(b'ply\nformat binary_little_endian 1.0\nelement vertex %d\n' % len(v))
    assert b'property list uchar int vertex_indices\nend_header\n' in head
    assert os.path.getsize(p) == head.index(b'end_header\n') + 11 + 12 * len(v) + 13 * len(t)
    e = str(tmp_path / 'e.ply')
    harness.write_ply(e, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))
    v3, t3 = harness.read_ply(e)
    assert v3.shape == (0, 3) and t3.shape == (0, 3)


def test_write_ply_refuses_bad_indices(tmp_path):
    from honerf_amd import harness
    with pytest.raises(ValueError):
        harness.write_ply(str(tmp_path / 'x.ply'), np.zeros((3, 3), np.float32), np.array([[0, 1, 3]]))

"""Hand-made inputs of the compatibility-graph tests (tests/test_simgraph_ref.py on the CPU, tests/test_gpu_simgraph.py on the
device). Data only, built with the helpers of tests/polymatch_cases.py; the expected results come from tests/simgraph_ref.py
and, for weights_scene, from the figures worked out in tests/test_simgraph_ref.py."""
from polymatch_cases import hline, make_scene, make_seeds


def weights_scene():
    """3 views of 200 x 150 (no line and no observation on a 10 px cell boundary). Every view: 0 a line at y = 41, 1 a line
    at y = 45 that ends at x = 60 (both within 10 px of a point at x = 33), 2 a line at y = 101; view 2 also has 3, a line
    at y = 48 that ends at x = 60.
      point 0  views 0, 1 at (103, 43): (0,0) (1,0)                              weight 2 / 2
      point 1  views 0, 1 at (103, 71): nothing                                  weight 0
      point 2  view 0 at (33, 43), view 1 at (103, 43): (0,0) (0,1) (1,0)        weight 2 / 3, an edge inside view 0
      point 3  views 0, 1 at (103, 43), view 2 at (103, 99): (0,0) (1,0) (2,2)   weight 3 / 3
      point 4  view 0, then view 1 twice: the last observation (103, 43) counts for both entries: (0,0) (1,0), weight 2 / 2
      point 5  views 0, 1, 2 at (33, 43): (0,0) (0,1) (1,0) (1,1) (2,0) (2,1) (2,3)   weight 3 / 7"""
    base = [hline(41, 10, 190, 4), hline(45, 10, 60, 3), hline(101, 10, 190, 4)]
    sc = make_scene(3, 200, 150, [base, base, base + [hline(48, 10, 60, 3)]])
    T = [
        [(0, 103, 43), (1, 103, 43)],
        [(0, 103, 71), (1, 103, 71)],
        [(0, 33, 43), (1, 103, 43)],
        [(0, 103, 43), (1, 103, 43), (2, 103, 99)],
        [(0, 103, 43), (1, 103, 71), (1, 103, 43)],
        [(0, 33, 43), (1, 33, 43), (2, 33, 43)],
    ]
    return sc, make_seeds(T)


def long_polyline_scene():
    """3 views of 800 x 100, polyline 0 of every view a line at y = 51 from x = 10 to 790; view 2 also has polyline 1, a short
    line at y = 56 for x in 10..120 (the first eleven points find two polylines there: their weight is 3 / 4, the others'
    3 / 3). No line and no observation lies on a 10 px cell boundary.
      points 0..69   at x = 15.5 + 11 i, 2 px from the line in views 0, 1, 2
      points 70..74  close to the line in view 0, 30 px from it in view 1: in A of the edge (0,0)-(1,0), not in B
      points 75..79  views 0 and 2 only: close to (0,0), their tracks do not list view 1, so they are in neither list
    close_refpoints of (0,0) has 80 points; A and B of the edge (0,0)-(1,0) have 75 and 70."""
    line = hline(51, 10, 790, 14)
    sc = make_scene(3, 800, 100, [[line], [line], [line, hline(56, 10, 120, 3)]])
    T = [[(0, 15.5 + 11 * i, 53), (1, 15.5 + 11 * i, 53), (2, 15.5 + 11 * i, 53)] for i in range(70)]
    T += [[(0, 23 + 150 * i, 49), (1, 23 + 150 * i, 81)] for i in range(5)]
    T += [[(0, 33 + 140 * i, 49.5), (2, 33 + 140 * i, 49.5)] for i in range(5)]
    return sc, make_seeds(T)


def order_scene():
    """The polylines of weights_scene with four points whose weights are 1, 2 / 3, 2 / 3 and 3 / 7, in this order. The edge
    (0,1)-(1,0) has B = all four and A = the last three: both of its sums change their float bits when the points are added
    in descending order."""
    sc, _ = weights_scene()
    T = [
        [(0, 103, 43), (1, 103, 43)],
        [(0, 33, 43), (1, 103, 43)],
        [(0, 33, 43), (1, 103, 43)],
        [(0, 33, 43), (1, 33, 43), (2, 33, 43)],
    ]
    return sc, make_seeds(T)

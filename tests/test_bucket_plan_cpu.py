"""run_bucket's planning without a GPU (siddhi_amd/csrc/sh_bucket_plan.h): which
select value is a consumer column and which rides the match stream, and whether
the carry kernels take the select's aggregates -- their sides, the e1 column, the
two e2 columns with the 8-byte one kept in slot 0 and the staged columns they
append. tests/bucket_plan builds the header with g++ and prints the plans of
hand-filled programs; the expectations below are derived from the rules of the
header, case by case.

Attributes: 0 = the partition attribute (a string unless said), 1 = price, 2 =
volume long; the matcher stages attribute 1 unless said. kind 1 = consumer column,
0 = match-stream column ms_of; side 0 = e1, 1 / 2 = e2 column 0 / 1, 3 = none."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))

EXPECTED = """
c2_agg select=ok ms=1 kind=1,1,0,1,1 ms_of=-1,-1,0,-1,-1
c2_agg carry=carry staged=1,2 widths=4,8 n=4 kind=sum,avg,count,sum side=2,0,3,1 e1=0:float e2[0]=1:long e2[1]=0:float agg_of=-1,0,1,2,3
c2_agg_double select=ok ms=1 kind=1,1,0,1,1 ms_of=-1,-1,0,-1,-1
c2_agg_double carry=none staged=1 widths=8
two_8byte_e2 select=ok ms=- kind=1,1 ms_of=-1,-1
two_8byte_e2 carry=none staged=1,2,3 widths=4,8,8
two_4byte_e1 select=ok ms=1,3 kind=0,0 ms_of=0,1
two_4byte_e1 carry=none staged=1 widths=4
same_e1_twice select=ok ms=1 kind=0,0 ms_of=0,0
same_e1_twice carry=carry staged=1 widths=4 n=2 kind=sum,avg side=0,0 e1=0:float e2[0]=-1 e2[1]=-1 agg_of=0,1
five_aggregates select=ok ms=- kind=1,1,1,1,1 ms_of=-1,-1,-1,-1,-1
five_aggregates carry=none staged=1 widths=4
bool_argument select=ok ms=- kind=1 ms_of=-1
bool_argument carry=none staged=1 widths=4
count_alone select=ok ms=- kind=1 ms_of=-1
count_alone carry=carry staged=1 widths=4 n=1 kind=count side=3 e1=-1 e2[0]=-1 e2[1]=-1 agg_of=0
staged_full select=ok ms=- kind=1 ms_of=-1
staged_full carry=na staged=1,2,3,4 widths=4,8,4,4
staged_full_among select=ok ms=- kind=1 ms_of=-1
staged_full_among carry=carry staged=1,2,3,4 widths=4,8,4,4 n=1 kind=sum side=1 e1=-1 e2[0]=2:int e2[1]=-1 agg_of=0
five_e1_values select=na
float_partition select=ok ms=0 kind=0,1 ms_of=0,-1
""".strip().split("\n")


def test_bucket_plans_of_hand_filled_programs():
    d = os.path.join(HERE, "bucket_plan")
    subprocess.run(["make", "-s", "-C", d], check=True)
    r = subprocess.run([os.path.join(d, "bucket_plan")], capture_output=True, text=True, timeout=60, check=True)
    got = [line for line in r.stdout.split("\n") if line]
    for g, e in zip(got, EXPECTED):
        assert g == e
    assert len(got) == len(EXPECTED)

"""Writes tests/golden/mednet_train_graph.json: the TOPOLOGY of the reference's own training net -- which layers the TRAIN phase
holds, of which type, wired through which blobs, with which layer parameters -- read out of the reference's project file
/root/reference/projects/videovec_embedding/mednet_embedding_train.prototxt (a model definition, i.e. data; the file itself is not
copied).  The fixture is what pins the WIRING of the assembled graph to the reference: tests/test_oracle_graph_topology.py executes
it layer by layer with the oracle's (separately pinned) layer functions and compares with the oracle's assembled step, and checks that
the product's generator (videovector_amd/prototxt.py) produces exactly this graph.  Run in the build container (the reference tree is
not on the GPU box):  python tests/golden/make_graph_golden.py
It also writes tests/golden/shipped_solver.json, the field values of the reference's solver file (mednet_embedding_train_solver.prototxt),
from which tests/test_facade_proto.py rebuilds that file's settings for the facade's parser.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from prototxt_parse import parse_prototxt, train_topology   # noqa: E402  (tests/prototxt_parse.py)

REF = "/root/reference/projects/videovec_embedding/mednet_embedding_train.prototxt"
REF_SOLVER = os.path.join(os.path.dirname(REF), "mednet_embedding_train_solver.prototxt")

if __name__ == "__main__":
    net = parse_prototxt(open(REF).read())
    topo = train_topology(net)
    topo["_source"] = "projects/videovec_embedding/mednet_embedding_train.prototxt (TRAIN phase), via tests/golden/make_graph_golden.py"
    topo["test_layers"] = train_topology(net, "TEST")["layers"]       # the TEST phase of the same file (the extraction / retrieval branch)
    json.dump(topo, open(os.path.join(HERE, "mednet_train_graph.json"), "w"), indent=1, sort_keys=True)
    print("%d TRAIN layers, %d TEST layers" % (len(topo["layers"]), len(topo["test_layers"])))
    text = open(REF_SOLVER).read()
    fields = {k: v[0] for k, v in parse_prototxt(text).items()}
    solver = {"_source": "projects/videovec_embedding/mednet_embedding_train_solver.prototxt, via tests/golden/make_graph_golden.py",
              "fields": fields,
              "enum_fields": [k for k, v in fields.items() if isinstance(v, str) and '%s: "%s"' % (k, v) not in text]}
    json.dump(solver, open(os.path.join(HERE, "shipped_solver.json"), "w"), indent=1)
    print("%d solver fields" % len(fields))

"""Each graph section of the Tacotron models is written once and shared by training and synthesis.

The three model files are parsed, not imported: a section that is copied again (a second walk over a convolution stack,
a second encoder in the synthesis file) brings its variable scope along as a second string constant.
"""
import ast
import os

import pytest

MODELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "nspeech_amd", "models")
FILES = ("tacotron2.py", "tacotron2_infer.py", "tacotron.py")

# literal -> how often it may stand in the three files together, and why
ALLOWED = {
    "encoder/conv_%d": 1,                        # the encoder stack's description; both walkers format it
    "decoder_postnet/postnet_conv_%d": 1,        # the postnet stack's description
    "expand/conv_%d": 1,                         # the expand stack's description
    "encoder/encoder_lstm": 1,                   # the encoder stack's description names the BiLSTM on top of it
    "expand/encoder_lstm": 1,                    # the expand stack's description does
    "decoder_postnet/dense/kernel": 1,           # one helper hands the offset to the shared tail and to backward()
    "attention_decoder/memory_layer/kernel": 1,  # named once on the base class: both models' encoders and both
                                                 # backward passes read that name
    "encoder_cbhg": 1,                           # Tacotron-1 names its CBHG scopes once; the shadows and the shared
    "post_cbhg": 1,                              # encoder / tail read the names
}


@pytest.fixture(scope="module")
def trees():
    out = {}
    for name in FILES:
        with open(os.path.join(MODELS, name)) as f:
            out[name] = ast.parse(f.read(), name)
    return out


@pytest.mark.parametrize("literal", sorted(ALLOWED))
def test_scope_is_written_once(trees, literal):
    where = [(name, node.lineno) for name, tree in trees.items() for node in ast.walk(tree)
             if isinstance(node, ast.Constant) and node.value == literal]
    assert len(where) == ALLOWED[literal], "%r stands at %s" % (literal, where)


def test_synthesis_file_calls_the_shared_sections(trees):
    """tacotron2_infer.py keeps the decoders and the graph capture: no embedding, no convolution layer of its own."""
    calls = [(node.func.attr, node.lineno) for node in ast.walk(trees["tacotron2_infer.py"])
             if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)]
    own = [c for c in calls if c[0] in ("embedding_fwd", "_conv_fwd")]
    assert not own, own

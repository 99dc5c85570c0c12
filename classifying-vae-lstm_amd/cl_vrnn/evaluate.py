"""Classifying VAE+LSTM -- scoring CLI (no counterpart in the reference, whose cl_vrnn/train.py builds the test split and
never uses it): the importance-weighted log-likelihood per window and per frame and Keras evaluate() of a
trained model on one split, with the windows built exactly as train.py builds its inputs.  One process, one GPU."""
import json
import os
import sys

if __package__ in (None, ''):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import clvae_amd  # noqa: E402,F401
from clvae_amd.cl_vrnn.model import load_model  # noqa: E402
from clvae_amd.cli import parser_for, score_split  # noqa: E402
from clvae_amd.utils.model_utils import to_categorical  # noqa: E402
from clvae_amd.utils.pianoroll import PianoData  # noqa: E402


def split_windows(P, split, margs):
    """(x, y) of one split as train.py hands them to fit(): inputs [y, x] (current frames, history) with --use_x_prev,
    else x; targets [recon, w, w, recon]."""
    w = to_categorical(getattr(P, split + '_song_keys'), margs['n_classes'])
    cur, hist = getattr(P, 'y_' + split), getattr(P, 'x_' + split)
    x = [cur, hist] if margs['use_x_prev'] else hist
    return x, [cur, w, w, cur]


def evaluate(args):
    margs = json.load(open(args.model_file.replace('.h5', '.json')))
    model, _, margs = load_model(args.model_file, batch_size=margs['batch_size'], seq_length=margs['seq_length'])
    P = PianoData(args.train_file, batch_size=margs['batch_size'], seq_length=margs['seq_length'], step_length=1,
                  return_y_next=margs['predict_next'] or margs['use_x_prev'], return_y_hist=True, squeeze_x=False,
                  squeeze_y=False, lazy=True)
    x, y = split_windows(P, args.split, margs)
    return score_split(model, x, y, args, margs)


def build_parser():
    return parser_for('cl_vrnn.evaluate')


if __name__ == '__main__':
    evaluate(build_parser().parse_args())

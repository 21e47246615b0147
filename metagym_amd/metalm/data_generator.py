"""Write MetaLM rows in the reference's text format (metagym/metalm/data_generator.py, plus --seed and --device):

    python -m metagym_amd.metalm.data_generator --samples 100 --output data.txt [--seed 0]

Without --seed the rows continue numpy.random's global stream (unseeded, as the reference's script runs); with it, row t
comes from numpy.random.seed(seed + t)."""
import argparse
import sys

from .metalm import MetaLM


def main(argv=None):
    parser = argparse.ArgumentParser(description="MetaLM data generator")
    parser.add_argument('--vocab_size', type=int, default=64)
    parser.add_argument('--elements_length', type=int, default=64)
    parser.add_argument('--elements_number', type=int, default=10)
    parser.add_argument('--error_rate', type=float, default=0.10)
    parser.add_argument('--sequence_length', type=int, default=4096)
    parser.add_argument('--samples', type=int, default=100)
    parser.add_argument('--output', type=str, default=None)
    parser.add_argument('--seed', type=int, default=None)
    parser.add_argument('--device', type=str, default="cuda")
    args = parser.parse_args(argv)
    dataset = MetaLM(V=args.vocab_size, n=args.elements_number, l=args.elements_length, e=args.error_rate,
                     L=args.sequence_length, device=args.device)
    dataset.generate_to_file(args.samples, sys.stdout if args.output is None else args.output, seed=args.seed)


if __name__ == "__main__":
    main()

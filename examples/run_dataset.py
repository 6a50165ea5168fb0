#!/usr/bin/env python3
"""End to end on one MI355X: a MALLET-style text file (one document per line: name, label, text) through the restated
front-end (LDAUtils.loadDataset), the sampler mirror (tui/ParallelLDA.java:170-296: setRandomSeed, addInstances, sample)
and the driver's output files (LDAUtils.java:1120-1254 formats).  Not a CLI: the reference's configuration parsing and
command line stay in Java (out of scope); this is the order of calls a caller makes.

    python examples/run_dataset.py tests/golden/datasets/cats.txt --topics 20 --iterations 200 --out /tmp/cats_run
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from ldagroupedgibbssampler_amd.native import SCHEME_FLAGS

    ap = argparse.ArgumentParser()
    ap.add_argument("dataset")
    ap.add_argument("--stoplist", default=None, help="one stop word per line (LDAConfiguration: stoplist.txt)")
    ap.add_argument("--rare-threshold", type=int, default=0)
    ap.add_argument("--scheme", default="ggs", choices=list(SCHEME_FLAGS) + ["spalias_priors", "lightpcldaw2"])   # spalias_priors: spalias's flag and --topic-priors; lightpcldaw2: its class, below
    ap.add_argument("--topic-priors", default=None, metavar="FILE",
                    help="scheme spalias_priors: lines `topic,word,word,...`; those words may only belong to that topic (topic_prior_filename)")
    ap.add_argument("--vs-prior", type=float, default=0.5, metavar="X",
                    help="scheme nzvsspalias: the prior probability that a cell without tokens stays in its topic (variable_selection_prior)")
    ap.add_argument("--topics", type=int, default=20)
    ap.add_argument("--alpha", type=float, default=0.1)
    ap.add_argument("--beta", type=float, default=0.01)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--optimize-interval", type=int, default=-1, metavar="N",
                    help="hyperparam_optim_interval (MALLET's --optimize-interval): alpha and beta are re-estimated every N iterations, N > 1")
    ap.add_argument("--symmetric-alpha", action="store_true", help="symmetric_alpha: one concentration for all topics instead of an alpha per topic")
    ap.add_argument("--seed", type=int, default=4711)
    ap.add_argument("--top-words", type=int, default=8, help="nr_top_words: words per topic, printed and in TopWords.txt / RelevanceWords.txt (clamped to the vocabulary size, as the driver clamps)")
    ap.add_argument("--lambda", dest="lambda_", type=float, default=0.6, help="lambda: the relevance weight of RelevanceWords.txt")
    ap.add_argument("--doc-topic-distances", action="store_true",
                    help="compute_doc_topic_distances: min_doc_distances.csv and min_topic_distances.csv in --out, one line per iteration from --start-diagnostic on")
    ap.add_argument("--start-diagnostic", type=int, default=500, help="start_diagnostic: first iteration of the log posterior and the distances")
    ap.add_argument("--topic-diagnostics", default=None, metavar="FILE",
                    help="save_doc_topic_diagnostics / doc_topic_diagnostics_filename: TopicModelDiagnosticsPlain's CSV (eleven quality scores per topic) "
                         "as FILE in --out; the coherence column is printed")
    ap.add_argument("--similarity", default=None, metavar="TESTFILE",
                    help="tui/LDASimilarity: fold the documents of TESTFILE (read against the training alphabet) into the trained Phi and write "
                         "nearest_documents.csv into --out: lines `query_name,rank,train_name,distance`, the --nearest nearest training documents "
                         "of every test document (the reference only prints to stdout: the file format is this project's)")
    ap.add_argument("--distance", default="KLDistance", help="the Java class name of the distance (cc/mallet/similarity), e.g. ManhattanDistance")
    ap.add_argument("--nearest", type=int, default=1, help="training documents per test document, 1 .. 16")
    ap.add_argument("--fold-in", type=int, default=2000,
                    help="z-only sweeps of the test documents under the trained Phi (LDADistancer.java:62).  The fold-in sampler is built from the "
                         "configuration, as in Java: with --optimize-interval the training rows use the learned alpha, the test rows --alpha")
    ap.add_argument("--out", default=None, help="directory for the driver's files (phi / theta / counts / likelihood / TopWords.txt / RelevanceWords.txt)")
    args = ap.parse_args()
    if args.topic_priors and args.scheme != "spalias_priors":
        ap.error("--topic-priors belongs to --scheme spalias_priors")
    if args.topic_diagnostics and not args.out:
        ap.error("--topic-diagnostics writes into --out")
    if args.similarity and not args.out:
        ap.error("--similarity writes into --out")
    if args.similarity and args.scheme in ("collapsed", "lightcollapsed", "adlda"):
        ap.error("--similarity folds the test documents into a drawn Phi: scheme %s has none" % args.scheme)

    from ldagroupedgibbssampler_amd import formats as F
    from ldagroupedgibbssampler_amd.frontend import load_dataset
    from ldagroupedgibbssampler_amd.sampler import SimpleLDAConfiguration, create_model

    ds = load_dataset(args.dataset, stoplist=args.stoplist, rare_threshold=args.rare_threshold)
    c = ds.corpus
    print("%s: %d documents, %d types, %d tokens" % (os.path.basename(args.dataset), c.num_docs, c.num_types, c.num_tokens))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    cfg = SimpleLDAConfiguration(scheme=args.scheme, topics=args.topics, alpha=args.alpha, beta=args.beta, iterations=args.iterations,
                                 seed=args.seed, exec_time=None, compute_likelihood=bool(args.out), log_dir=args.out,
                                 topic_prior_filename=args.topic_priors, variable_selection_prior=args.vs_prior,
                                 hyperparam_optim_interval=args.optimize_interval, symmetric_alpha=args.symmetric_alpha,
                                 compute_doc_topic_distances=args.doc_topic_distances, start_diagnostic=args.start_diagnostic,
                                 nr_top_words=args.top_words, save_doc_topic_diagnostics=bool(args.topic_diagnostics),
                                 doc_topic_diagnostics_filename=args.topic_diagnostics, **{"lambda": args.lambda_})
    if args.scheme == "nzvsspalias":                          # not in create_model's registry: the class itself
        from ldagroupedgibbssampler_amd.sampler import NZVSSpaliasUncollapsedParallelLDA
        model = NZVSSpaliasUncollapsedParallelLDA(cfg)
    elif args.scheme == "adlda":
        from ldagroupedgibbssampler_amd.sampler import ADLDA
        model = ADLDA(cfg)
    elif args.scheme == "lightpcldaw2":
        from ldagroupedgibbssampler_amd.sampler import LightPCLDAtypeTopicProposal
        model = LightPCLDAtypeTopicProposal(cfg)
    else:
        model = create_model(cfg)
    model.setRandomSeed(cfg.get_seed())
    model.addInstances(c)
    model.sample(args.iterations)
    print("%d iterations: z %.1f ms, Phi %.1f ms in all; model log likelihood %.2f" %
          (model.getCurrentIteration(), model.zSamplingTimeCum, model.phiSamplingTimeCum, model.modelLogLikelihood()))

    print("alpha: %s (sum %.17g)\nbeta: %.17g" % (" ".join("%.6g" % a for a in model.getAlpha()), model.alphaSum, model.getBeta()))

    requested = min(cfg.nr_top_words, c.num_types)          # tui/ParallelLDA.java:272-274
    top = model.getTopWords(requested)                      # LDAUtils.getTopWords on the device-resident counts: ties by falling id
    for k in range(args.topics):
        print("topic %2d: %s" % (k, " ".join(top[k])))

    if args.out:
        K, V, D, it = args.topics, c.num_types, c.num_docs, model.getCurrentIteration()
        n_wk = np.asarray(model.getTypeTopicMatrix())       # [V][K] counts, for type_topic_counts.csv
        F.write_top_words(top, os.path.join(args.out, "TopWords.txt"))
        F.write_top_words(model.getTopRelevanceWords(requested, cfg.lambda_), os.path.join(args.out, "RelevanceWords.txt"))
        if cfg.save_doc_topic_diagnostics:                  # tui/ParallelLDA.java:218-225, with nr_top_words clamped first
            tmd = model.getTopicModelDiagnostics(requested)
            F.write_topic_diagnostics(tmd.names, [tmd.scores[x] for x in tmd.names], os.path.join(args.out, cfg.doc_topic_diagnostics_filename))
            print("coherence: %s" % " ".join("%d:%s" % (k, F.java_format_fixed(v, 4)) for k, v in enumerate(tmd.scores["coherence"])))
        if args.scheme != "collapsed":
            F.write_binary_double_matrix(np.asarray(model.getPhi()), F.binary_matrix_name(os.path.join(args.out, "phi"), K, V, it))
        F.write_ascii_double_matrix(np.asarray(model.getThetaEstimate()), F.ascii_matrix_name(args.out, "Theta_DxK", D, K, it))
        F.write_ascii_int_matrix(n_wk.T, os.path.join(args.out, "type_topic_counts.csv"))
        with open(os.path.join(args.out, "hyperparameters.txt"), "w") as f:       # the final values, every digit: alpha per topic, then beta and betaSum
            f.write("".join("alpha\t%d\t%.17g\n" % (k, a) for k, a in enumerate(model.getAlpha())))
            f.write("beta\t%.17g\nbetaSum\t%.17g\n" % (model.getBeta(), model.betaSum))
        if args.similarity:
            from ldagroupedgibbssampler_amd.similarity import LDADistancer
            test = load_dataset(args.similarity, stoplist=args.stoplist, alphabet=tuple(c.vocab))   # a tuple: the alphabet does not grow (data_alphabet)
            distancer = LDADistancer(cfg)
            distancer.setDist(args.distance)
            distancer.setTrainedSampler(model)              # the model just trained, whatever its scheme; the fold-in is spalias's
            idx, dist = distancer.nearest(test.corpus, args.nearest, fold_in_sweeps=args.fold_in)
            with open(os.path.join(args.out, "nearest_documents.csv"), "w") as f:
                for q, name in enumerate(test.names):
                    for r in range(args.nearest):
                        if idx[q, r] >= 0:
                            f.write("%s,%d,%s,%s\n" % (name, r, ds.names[idx[q, r]], F.java_double_to_string(dist[q, r])))
        print("wrote", ", ".join(sorted(os.listdir(args.out))))


if __name__ == "__main__":
    main()

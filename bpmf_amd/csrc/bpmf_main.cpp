// bpmf_main.cpp -- the `bpmf` executable of this repo: the reference's command line, stdout lines
// and output files (c++/bpmf.cpp:41-260) on top of libbpmf_hip.so.
//
// Host C++ only: it reads the matrices (io.cpp), mirrors them to the device through the C ABI of
// include/bpmf_hip.h and runs main()'s Gibbs loop; every column update happens in the HIP kernels.
// Flags: -n TRAIN -p TEST [-o DIR] [-i N] [-b N] [-a F] [-d K] [-t N] [-f N] [-k] [-r] [-v] [-g N] [--fp32]
// -g N (or BPMF_NGPU=N): N GPUs of this node, the job of `mpirun -np N bpmf` (c++/bpmf.cpp:111-117, c++/mpi_common.h:14-50):
// one host thread + one context per GPU in this process, RCCL id shared in memory, columns of both sides sharded,
// `nprocs: N`, every rank writes bpmf_<rank>.out like the reference's ranks do.
// -m / -l "MU_FILE,LAMBDA_FILE": propagated posteriors of a previous run (c++/bpmf.cpp:134-135).
// K (the reference's compile-time BPMF_NUMLATENT, c++/bpmf.h:22-24; ci/multilatent.sh:5 builds bpmf-8 ... bpmf-128 incl. 10, 20 ...
// 100) is chosen at run time: -d K, else the environment variable BPMF_NUMLATENT, else 32.  Any 1 <= K <= 128, always in the
// reference's fp64 arithmetic.  --fp32 (or BPMF_HIP_F32=1; K > 64 only) opts into the library's mixed-precision large-K path
// and says so on stdout: never chosen silently.
// --topn N (with -o DIR, one GPU): the N unrated items of every user with the highest posterior-mean prediction over the kept
// samples, and its spread, to DIR/topn.csv (query,rank,candidate,mean,std; 1-based ids in the numbering of the input);
// --topn-by cols ranks the users of every item instead.  stdout is the same as without it.
// --intervals L1[,L2..] (1 <= -i - -b <= 4096, a test matrix; one GPU, no -g): predictive intervals and their calibration (DESIGN.md
// section 31).  The run keeps the sample rings of both sides (the blocking loop) and after the chain bpmf_hip_interval_cells gives every
// test cell the central intervals of its posterior predictive mixture at the 1 .. 4 levels and the probability integral transform of
// its held-out value: two more Final lines (coverage, PIT) and, with -o DIR, DIR/intervals.csv (row,col,value,mean,std,pit,lo<L>,hi<L>,..;
// 1-based original ids in test-set order).  With --model DIR --predict FILE the same file for FILE's cells, FILE's values being the
// observations.
// --loo (2 <= -i - -b <= 4096; one GPU, no -g): PSIS-LOO cross-validation of the training cells.  The run keeps
// the sample rings of both sides (the blocking loop) and after the chain bpmf_hip_loo_cells gives every training cell its leave-one-out
// log predictive density by Pareto-smoothed importance sampling and the diagnostic khat: one more Final line and, with -o DIR,
// DIR/loo-elpd.sdm and DIR/loo-khat.sdm in the training matrix's numbering.  With --model DIR -n TRAIN the same for TRAIN's cells.
// --topn-score ucb|prob|ei ranks by an acquisition score of the kept samples instead of their mean:
// mean + kappa std (--topn-kappa), the posterior probability that a rating exceeds --topn-threshold, or the expected excess over
// it, with sigma = 1 / sqrt(-a) (1 under --probit); topn.csv then has the columns query,rank,candidate,score,mean,std.
// --noise adaptive (one GPU, no -g): the noise precision is sampled after every iteration from its Gamma posterior (prior
// --alpha-prior A0,B0, default 1,1; cap --alpha-max F), -a is its initial value; every iteration line then ends with the alpha
// it ran with and the training RMSE after it, and -o DIR also gets DIR/alpha.csv.
// --probit [--probit-threshold F] (one GPU, no -g): the ratings are labels (positive if > F, default 0.5) under the probit
// likelihood: mean rating 0, alpha 1, latent scores redrawn on the device ahead of every sampler launch.
// After "Final Avg RMSE" the run prints "Final AUC" and "Final Brier" of the posterior-mean probabilities of the test entries,
// and -o DIR also gets DIR/probit.csv (row,col,label,prob).  Without these flags nothing changes.
// --ordinal [--ordinal-levels a,b,..] [--ordinal-cutpoints g1,..] [--ordinal-step F] (one GPU, no -g): the ratings are ordered
// categories under the ordinal probit likelihood: mean rating 0, alpha 1, latent scores between the cutpoints
// of their level redrawn on the device ahead of every sampler launch, the cutpoints sampled by one Metropolis-Hastings step per
// iteration (or fixed).  After "Final Avg RMSE" the run prints "Final ordinal RMSE", "Final accuracy" and "Final log-prob" over the
// test entries, and -o DIR also gets DIR/ordinal.csv (row,col,value,expected,p1..pC) and DIR/cutpoints.csv (iteration,accepted,step,g1..).
// --new-row-features FILE / --new-col-features FILE (with the matching --row-features / --col-features, -o DIR, -i > -b): users /
// movies that are NOT in the training matrix, predicted from their features alone: DIR/new-rows-mean.ddm,
// new-rows-std.ddm (new x movies), new-cols-mean.ddm, new-cols-std.ddm (users x new); with --topn N also DIR/new-rows-topn.csv /
// new-cols-topn.csv.  std does not include the observation noise 1 / alpha.
// --fold-in-rows FILE / --fold-in-cols FILE (with -o DIR, -i > -b; one GPU, no -g): users / movies that arrive after training with a
// few ratings and no features.  FILE is a sparse matrix, new users x movies / users x new movies, oriented as the
// training matrix.  After the chain every kept sample gives one draw of their factors from their conditional given that sample of the
// other side (bpmf_hip_foldin): DIR/foldin-rows-mean.ddm, foldin-rows-std.ddm (new x movies), foldin-cols-mean.ddm, foldin-cols-std.ddm
// (users x new); with --topn N also DIR/foldin-rows-topn.csv / foldin-cols-topn.csv, the new entities as the queries, their own
// ratings excluded.  One more header line names the counts; everything else keeps its format.
// --save-model DIR (-i > -b; one GPU, no -g): the run keeps the sample rings of both sides and, unless --probit, both hyper rings, and
// writes them after the chain as a model directory, format version 1 (include/bpmf_io.h): model.txt,
// U-samples.ddm, V-samples.ddm, U-hyper.ddm, V-hyper.ddm, in the numbering of the input.  One more header line, `save-model: DIR`.
// --similar N (with -o DIR, one GPU, no -g): the N nearest neighbours of every item (--similar-by cols, the default) or user (rows)
// among the entities of the same side, by the posterior mean of the per-sample cosine (--similar-kind euclid: negative squared
// distance) minus --similar-kappa times its spread, to DIR/similar-cols.csv / similar-rows.csv; entities with
// fewer than --similar-min-ratings training ratings are not listed.  Also served from --model DIR.  stdout is the same as without it.
// --diagnose (-i - -b in 8 .. 4096; one GPU, no -g): convergence diagnostics of the test predictions.  The run keeps
// the sample rings of both sides (the blocking loop) and after the chain bpmf_hip_diag_cells gives every test cell its split-Rhat and
// effective sample size (ESS) over the kept samples; one more header line, four more Final lines (ESS, split-Rhat, MCSE/std, and the ESS
// of the post-burn-in traces of RMSE, FU and FM), and with -o DIR also DIR/diagnostics.csv: row,col,mean,std,rhat,ess,mcse, 1-based
// original ids in test-set order.  With --model DIR --predict FILE the same file is written for FILE's cells, without the trace line.
// --score (-i - -b >= 2; one GPU, no -g): model comparison.  The run keeps the sample rings of both sides (the
// blocking loop) and after the chain bpmf_hip_score_cells gives every test cell the log of its posterior predictive density at the
// held-out value and every training cell the same with its WAIC correction, under the likelihood of the run (Gaussian with the
// alpha of every kept iteration, the run's weights and censoring flags; Student-t under --robust; probit); one more header line, two
// more Final lines (test log-density, WAIC), and with -o DIR also DIR/score.csv (row,col,value,lpd,mean,std; 1-based original ids in
// test-set order) and DIR/waic-elpd.sdm (lpd - var of every training cell).  With --model DIR --predict FILE the values of FILE are
// the observations (score.csv and the first line); with -n TRAIN also the WAIC of TRAIN's cells.
// --model DIR -o OUT [-n TRAIN] [-p TEST]: no chain runs (run_model).  The model is loaded into a fp64 context and serves --predict FILE
// [--predict-threshold F] (OUT/predict.csv: row,col,mean,std[,prob] for the cells FILE lists, 1-based, in the reader's order; prob with
// sigma = 1 / sqrt(alpha), always there for a probit model with t = 0 unless given and sigma = 1), --topn N with its --topn-* flags and
// --rank-eval N -p TEST (both need -n TRAIN: the rated cells are what they exclude) and --fold-in-rows / --fold-in-cols FILE (a Gaussian
// model with hyper files), each with exactly the files of a training run.  stdout: one line `model: DIR, R x C, num_latent K, S samples,
// LIKELIHOOD` (and the Final rank lines of --rank-eval); times go to stderr.
// --row-features FILE / --col-features FILE [--lambda-beta F] (one GPU, no -g): side information.  FILE is a
// dense matrix (.ddm / .csv) with one row per user / movie; both sides then step through the blocking bpmf_hip_link_sample and
// -o DIR also gets DIR/U-link.ddm / DIR/V-link.ddm, the posterior mean of the link matrix (D x num_latent).  A sparse FILE (.sdm / .sbm /
// coordinate .mtx) of any width takes the CG draw of DESIGN.md section 14 (bpmf_hip_side_set_features_sparse; --link-tol, --link-max-iter).
// --lambda-beta-prior A0,B0: lambda_beta is sampled per side with features (bpmf_hip_side_link_lambda_prior), one
// more header line names the prior, and -o DIR also gets DIR/lambda_beta.csv (iteration,lambda_rows,lambda_cols).
// --censored FILE (one GPU, no -g): FILE is a sparse matrix of the training matrix's shape that lists the training cells whose value
// is only a bound: an entry > 0 = the true value is at least the recorded one, < 0 = at most (.sbm: every
// listed cell is a lower bound).  Both sides redraw the latent values of their censored cells on the device ahead of every sampler
// launch (bpmf_hip_side_set_censored); one more header line counts the bounds, everything else keeps its format.
// --weights FILE (one GPU, no -g): FILE is a sparse matrix of the training matrix's shape with a precision weight w > 0 for the
// training cells it lists: such a rating is observed with the precision alpha w, every other one with alpha.
// Both sides get their weights once (bpmf_hip_side_set_weights) and run the weighted form of their sampler; one more header line
// counts the weighted cells, everything else keeps its format.
// --robust NU (one GPU, no -g): Student-t noise with NU >= 1 degrees of freedom instead of Gaussian noise: both
// sides redraw a precision weight per rating on the device ahead of every sampler launch (bpmf_hip_side_set_robust); one more header
// line names NU, -o DIR also writes DIR/robust-weights.sdm (the posterior-mean weight of every training cell), everything else keeps
// its format.
// --implicit W0 [--weights FILE] (one GPU, no -g): implicit feedback: every cell the training matrix does not
// store is a zero of weight W0, a stored cell has its value and the confidence 1 (or its entry of --weights FILE, > W0); mean rating 0.
// Both sides become implicit sides (bpmf_hip_side_set_implicit) and step through the blocking bpmf_hip_implicit_sample; one more header
// line, everything else keeps its format (the RMSE columns are over the -p cells as given).
// --rank-eval N [--rank-by rows|cols] [--rank-threshold F] (-i > -b, one GPU): after the chain every test cell with a value > F (default:
// every test cell, or value > 0 under --implicit) is ranked among the candidates its query has not rated in the training matrix, by the
// posterior-mean score of the kept samples (bpmf_hip_rank_eval).  After "Final Avg RMSE" the run prints "Final recall@N", "Final NDCG@N",
// "Final MRR", "Final MPR" and "Final rank AUC"; -o DIR also gets DIR/ranks.csv (query,candidate,rank,ncand).
// --tensor FILE.tns [--tensor-test FILE.tns] [--tensor-dims I,J,T] (one GPU, no -g): Bayesian CP factorisation of a sparse tensor of
// order 3 in the place of -n / -p.  FROSTT .tns files (one entry per line, "i j t value", 1-based, # comments,
// optional .gz); the sizes default to the largest index of either file.  -i, -b, -a, -d and -o apply.  stdout: the header line
// "tensor: I x J x T, NNZ ratings, NNZT test", one line per iteration (RMSE, avg RMSE, the norms F1 F2 F3 of the three factor
// matrices, items/sec), "Final Avg RMSE:".  -o DIR gets mode1-mu.ddm .. mode3-mu.ddm (the posterior-mean factors, num_latent x size)
// and Pavg.tns / Pm2.tns (the test entries in the order of their file, 1-based).
#include <getopt.h>
#include <fcntl.h>
#include <unistd.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <memory>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../include/bpmf_hip.h"
#include "io.h"
#include "../../include/bpmf_io.h"

namespace {

using bpmf::io::Csc;
using bpmf::io::Dense;

double tick()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

void usage()
{
    std::cout << "Usage: bpmf -n <MTX> -p <MTX> [-o DIR/] [-i N] [-b N] [-f N] [-a F] [-d K] [-krv] [-t N] [-m MTX,MTX] [-l MTX,MTX] [-g N] [--fp32] [--topn N [--topn-by rows|cols] [--topn-score mean|ucb|prob|ei] [--topn-kappa F] [--topn-threshold F]]"
              << " [--noise fixed|adaptive [--alpha-prior A0,B0] [--alpha-max F]] [--probit [--probit-threshold F]] [--ordinal [--ordinal-levels a,b,..] [--ordinal-cutpoints g1,..] [--ordinal-step F]] [--censored FILE] [--weights FILE] [--robust NU] [--implicit W0] [--rank-eval N [--rank-by rows|cols] [--rank-threshold F]] [--fold-in-rows FILE] [--fold-in-cols FILE] [--save-model DIR] [--similar N [--similar-by cols|rows] [--similar-kind cosine|euclid] [--similar-kappa F] [--similar-min-ratings M]]\n"
              << "   or: bpmf --model DIR -o OUT [-n <train_matrix>] [-p <test_matrix>] [--predict FILE [--predict-threshold F]] [--topn N ...] [--rank-eval N ...] [--similar N ...] [--fold-in-rows FILE] [--fold-in-cols FILE]\n"
              << "       bpmf --tensor <TNS> [--tensor-test <TNS>] [--tensor-dims I,J,T] [-o DIR/] [-i N] [-b N] [-a F] [-d K]\n"
              << "\n"
              << "Parameters:\n"
              << "  -n MTX: training matrix (rows = users, columns = items)\n"
              << "  -p MTX: test matrix\n"
              << "  [-o DIR]: directory for the model and the predictions\n"
              << "  [-i N]: total number of Gibbs iterations (20)\n"
              << "  [-b N]: number of burn-in iterations (5)\n"
              << "  [-f N]: update frequency (accepted, unused)\n"
              << "  [-a F]: noise precision alpha (2.0)\n"
              << "  [-d K]: number of latent dimensions, 1 .. 128, fp64 (32, or $BPMF_NUMLATENT)\n"
              << "  [--fp32]: mixed-precision column update (fp32 factors / Gram / factorisation; K > 64 only; or BPMF_HIP_F32=1)\n"
              << "\n"
              << "  [-l MTX,MTX]: propagated posterior mu and Lambda matrices for U\n"
              << "  [-m MTX,MTX]: propagated posterior mu and Lambda matrices for V\n"
              << "\n"
              << "  [-g N]: shard users and items over N GPUs of this node (RCCL over xGMI; default $BPMF_NGPU or 1)\n"
              << "  [-k]: do not balance the item-to-GPU assignment on work (equal column counts per GPU instead)\n"
              << "  [-r]: redirect stdout to bpmf_<rank>.out (always with more than one GPU)\n"
              << "  [-v]: write every sample (U-<i>.ddm, V-<i>.ddm)\n"
              << "  [--topn N]: the N unrated items of every user with the highest posterior-mean prediction, with its standard\n"
              << "              deviation over the kept samples, to DIR/topn.csv (needs -o DIR; one GPU; 1 <= N <= 32)\n"
              << "  [--similar N [--similar-by cols|rows] [--similar-kind cosine|euclid] [--similar-kappa F] [--similar-min-ratings M]]: the N\n"
              << "              nearest neighbours of every item (cols, the default) or user (rows) among the entities of the same side, to\n"
              << "              DIR/similar-cols.csv / similar-rows.csv (query,rank,neighbour,score,mean,std): per kept sample the cosine between\n"
              << "              the two factor vectors (or, euclid, their negative squared distance) -- which no rotation of the latent space\n"
              << "              changes -- then score = mean - kappa std over the samples (kappa >= 0, default 0); entities with fewer than M\n"
              << "              training ratings are not listed (needs -o DIR and -i > -b; one GPU, no -g; 1 <= N <= 32; not with --tensor,\n"
              << "              -m / -l or BPMF_REDUCE=1; also served from --model DIR, where --similar-min-ratings needs -n TRAIN)\n"
              << "  [--diagnose]: split-Rhat and the effective sample size (ESS) of every test prediction over the kept samples, and of the\n"
              << "              post-burn-in traces of RMSE, FU and FM: four more Final lines and, with -o DIR, DIR/diagnostics.csv\n"
              << "              (row,col,mean,std,rhat,ess,mcse; mcse = std / sqrt(ess)).  Needs 8 <= -i - -b <= 4096; one GPU, no -g; not with\n"
              << "              --tensor, -m / -l or BPMF_REDUCE=1; with --model DIR --predict FILE: the same file for FILE's cells\n"
              << "  [--diagnose-rank]: --diagnose with the rank-normalised estimator over chains (Vehtari et al. 2021): rank-normalised split-Rhat,\n"
              << "              bulk and tail ESS; the Final lines read `Final ESS: bulk min .. tail min ..`, `Final rank-Rhat`, and the file is\n"
              << "              row,col,mean,std,rhat,ess_bulk,ess_tail,mcse.  Accepted wherever --diagnose is; --diagnose under --model D0,D1,..\n"
              << "              takes it by itself\n"
              << "  [--chain c]: chain c (0 .. 63) of the model: the same run with its random numbers taken at the half-iteration indices\n"
              << "              c * 1048576, .. (one process per chain and GPU, each with --save-model DIR_c; --model D0,D1,.. pools them: a\n"
              << "              directory name with a comma is not supported).  One GPU, no -g; -i <= 1048576; not with features, --ordinal,\n"
              << "              --bias, --implicit, --tensor, -m / -l or BPMF_REDUCE=1\n"
              << "  [--score]: model comparison: the log posterior predictive density of every test cell (a proper score of held-out data) and\n"
              << "              WAIC over the training cells, under the likelihood of the run: two more Final lines and, with -o DIR,\n"
              << "              DIR/score.csv (row,col,value,lpd,mean,std) and DIR/waic-elpd.sdm.  Needs -i - -b >= 2; one GPU, no -g; not with\n"
              << "              --tensor, --ordinal, --implicit, -m / -l or BPMF_REDUCE=1; with --model DIR --predict FILE: FILE's values are\n"
              << "              the observations, and -n TRAIN adds the WAIC of TRAIN's cells\n"
              << "  [--intervals L1[,L2..]]: predictive intervals: for every test cell the central intervals at the 1 .. 4 levels (in [0.01, 0.998],\n"
              << "              e.g. 0.5,0.9) of its posterior predictive, the mixture over the kept samples of N(prediction, 1 / alpha), and\n"
              << "              the probability integral transform (pit) of its held-out value: two more Final lines (the coverage and mean\n"
              << "              width per level, the Kolmogorov distance of the pits from uniform) and, with -o DIR, DIR/intervals.csv\n"
              << "              (row,col,value,mean,std,pit,lo<L>,hi<L>,..).  Needs 1 <= -i - -b <= 4096 and -p TEST; one GPU, no -g; not with\n"
              << "              --tensor, --ordinal, --probit, --implicit, --robust, -m / -l or BPMF_REDUCE=1; with --model DIR --predict FILE:\n"
              << "              the same file for FILE's cells, FILE's values being the observations\n"
              << "  [--loo]: PSIS-LOO cross-validation: for every training cell the log predictive density a model fitted without it would\n"
              << "              give it, by Pareto-smoothed importance sampling over the kept samples, and the diagnostic khat (<= 0.7: the\n"
              << "              estimate can be trusted): one more Final line (looic, elpd, p_loo, se, the share of cells with k > 0.7) and, with\n"
              << "              -o DIR, DIR/loo-elpd.sdm and DIR/loo-khat.sdm.  Needs 2 <= -i - -b <= 4096; one GPU, no -g; not with --tensor,\n"
              << "              --ordinal, --implicit, -m / -l or BPMF_REDUCE=1; with --model DIR it needs -n TRAIN (the cells)\n"
              << "  [--topn-by rows|cols]: rank items per user (rows, the default) or users per item (cols)\n"
              << "  [--topn-score mean|ucb|prob|ei]: what --topn ranks by (default mean).  ucb: mean + kappa std; prob: the posterior\n"
              << "              probability that a rating exceeds the threshold; ei: the expected excess over the threshold; the\n"
              << "              observation noise is sigma = 1 / sqrt(-a), 1 under --probit.  DIR/topn.csv then has the columns\n"
              << "              query,rank,candidate,score,mean,std\n"
              << "  [--topn-kappa F]: kappa of ucb (default 1; negative: a lower confidence bound)\n"
              << "  [--topn-threshold F]: the threshold of prob and ei, required with them; on the rating scale, or on the\n"
              << "              latent-score scale under --probit (0 is the natural value there)\n"
              << "  [--noise fixed|adaptive]: fixed: alpha = -a throughout (the default); adaptive: alpha is sampled after every\n"
              << "              iteration from its Gamma posterior given the training residuals, -a is its initial value (one GPU)\n"
              << "  [--alpha-prior A0,B0]: Gamma prior of the adaptive alpha, shape A0 > 0 and rate B0 >= 0 (1,1)\n"
              << "  [--alpha-max F]: cap of the adaptive alpha (none)\n"
              << "  [--probit]: probit likelihood for binary matrices: a rating is a label, positive if > the threshold; mean rating 0,\n"
              << "              alpha 1; prints Final AUC / Final Brier over the test matrix, -o DIR also gets DIR/probit.csv (one GPU, no -g)\n"
              << "  [--row-features FILE] [--col-features FILE]: side information: a dense matrix (.ddm / .csv) with one row of D features per\n"
              << "              user / movie; the prior mean of its factors becomes mu + beta^T f with a sampled link matrix beta (one GPU, no -g,\n"
              << "              not with --probit, --noise adaptive, --fp32, -m / -l or BPMF_REDUCE=1); -o DIR also gets DIR/U-link.ddm / V-link.ddm\n"
              << "              A sparse FILE (.sdm, .sbm = all ones, coordinate .mtx; optional .gz) may have any number of feature columns: beta\n"
              << "              is then drawn by conjugate gradients on the device, F^T F is never formed (a dense FILE keeps 1 .. 1024 columns)\n"
              << "  [--new-row-features FILE] [--new-col-features FILE]: users / movies that are not in the training matrix, one row of features\n"
              << "              each (the kind and the D of --row-features / --col-features, which it needs, with -o DIR and -i > -b): predicted from\n"
              << "              their features against every movie / user, to DIR/new-rows-mean.ddm, new-rows-std.ddm (new x movies) and\n"
              << "              DIR/new-cols-mean.ddm, new-cols-std.ddm (users x new); std leaves the observation noise 1 / alpha out.  With\n"
              << "              --topn N also DIR/new-rows-topn.csv / new-cols-topn.csv (--topn-by rows: the best columns of every new row, the\n"
              << "              best new columns of every row; cols: the columns are the queries); files of more than 2^28 cells need --topn\n"
              << "  [--fold-in-rows FILE] [--fold-in-cols FILE]: users / movies that arrive after training with a few ratings and no features: a\n"
              << "              sparse matrix (.sdm, coordinate .mtx; optional .gz), new users x movies / users x new movies, as the training\n"
              << "              matrix is oriented (needs -o DIR and -i > -b; one GPU, no -g; not with --probit, -m / -l, BPMF_REDUCE=1, features on\n"
              << "              the same side or a --topn-score other than mean).  Every kept sample gives one draw of their factors from their\n"
              << "              ratings: DIR/foldin-rows-mean.ddm, foldin-rows-std.ddm (new x movies), foldin-cols-mean.ddm, foldin-cols-std.ddm\n"
              << "              (users x new); std leaves the observation noise 1 / alpha out.  With --topn N also DIR/foldin-rows-topn.csv /\n"
              << "              foldin-cols-topn.csv: the best N for every new entity, its own ratings excluded; files of more than 2^28 cells\n"
              << "              need --topn\n"
              << "  [--save-model DIR]: keep the post-burn-in samples of both sides and (unless --probit) their hyper-parameters, and write\n"
              << "              them after the chain as a model directory (model.txt, U-samples.ddm, V-samples.ddm, U-hyper.ddm, V-hyper.ddm;\n"
              << "              needs -i > -b; one GPU, no -g; not with BPMF_REDUCE=1, --tensor, --ordinal, --implicit, features, -m / -l)\n"
              << "  --model DIR: serve a saved model without a chain (needs -o OUT; not with -i, -b, -a, -g, --save-model or any flag of the\n"
              << "              likelihood or the chain; -d must be the model's).  --predict FILE [--predict-threshold F]: OUT/predict.csv with\n"
              << "              row,col,mean,std[,prob] for the cells the sparse matrix FILE lists (its values are ignored); --topn N and\n"
              << "              --rank-eval N -p TEST with their flags and files (both need -n TRAIN: the rated cells are excluded);\n"
              << "              --fold-in-rows / --fold-in-cols FILE with their files (a Gaussian model saved with hyper files)\n"
              << "  [--link-tol F] [--link-max-iter N]: the stopping rule of that CG draw: relative residual (1e-6), most iterations (1000);\n"
              << "              need a sparse feature file\n"
              << "  [--lambda-beta F]: the fixed precision scale of the rows of beta, for both sides (5: a default, not a tuned number)\n"
              << "  [--lambda-beta-prior A0,B0]: sample lambda_beta per side with features from its Gamma conditional, prior shape A0 > 0 and\n"
              << "              rate B0 >= 0 (5e-4,5e-4 is a weak default, not a tuned number); --lambda-beta is then the initial value.  The\n"
              << "              first draws are large (the chain starts at beta = 0): give the burn-in (-b) some tens of iterations.  With\n"
              << "              -o DIR the value every iteration used goes to DIR/lambda_beta.csv (iteration,lambda_rows,lambda_cols)\n"
              << "  [--probit-threshold F]: the threshold between negative and positive labels (0.5)\n"
              << "  [--ordinal]: ordinal probit likelihood for ordered categories (star ratings): the ratings take one of 2 .. 16 levels, a\n"
              << "              rating at level c has a latent score between the cutpoints g_{c-1} and g_c, which are sampled too (Metropolis-\n"
              << "              Hastings, one pass over the ratings per iteration); mean rating 0, alpha 1; prints Final ordinal RMSE / Final\n"
              << "              accuracy / Final log-prob over the test matrix, -o DIR also gets DIR/ordinal.csv and DIR/cutpoints.csv (one GPU,\n"
              << "              no -g; not with --probit, --tensor, --weights, --robust, --censored, --fold-in-*, --noise adaptive, --row-features /\n"
              << "              --col-features, -m / -l or BPMF_REDUCE=1)\n"
              << "  [--ordinal-levels a,b,..]: the level values, increasing (default: the distinct training values)\n"
              << "  [--ordinal-cutpoints g1,..]: fixed cutpoints, one fewer than the levels (default: sampled, from Phi^-1 of the level frequencies)\n"
              << "  [--ordinal-step F]: the proposal step of the cutpoints (default: 1 / sqrt(nnz), adapted towards 35 % acceptance in the burn-in;\n"
              << "              start, target and schedule are defaults, not tuned numbers)\n"
              << "  [--censored FILE]: training cells whose value is only a bound: a sparse matrix of the training matrix's shape (.sdm,\n"
              << "              coordinate .mtx, .sbm = all lower bounds; optional .gz), an entry > 0 = the true value is at least the recorded\n"
              << "              one, < 0 = at most; every entry must be a cell of the training matrix.  The latent values of these cells are\n"
              << "              redrawn on the device in every half-iteration (one GPU, no -g; not with --probit, --noise adaptive,\n"
              << "              --row-features / --col-features, -m / -l or BPMF_REDUCE=1)\n"
              << "  [--weights FILE]: a precision weight per training rating: a sparse matrix of the training matrix's shape (.sdm, coordinate\n"
              << "              .mtx; optional .gz) whose entries w > 0 weight the ratings of their cells -- precision alpha w instead of alpha;\n"
              << "              every entry must be a cell of the training matrix, every other rating has weight 1 (one GPU, no -g; not with\n"
              << "              --probit, --censored, --noise adaptive, --row-features / --col-features, -m / -l, --fp32 or BPMF_REDUCE=1)\n"
              << "  [--robust NU]: Student-t noise with NU >= 1 degrees of freedom (1: Cauchy) instead of Gaussian noise, scale 1 / sqrt(alpha): a\n"
              << "              precision weight per training rating is redrawn on the device in every half-iteration, so that a gross outlier\n"
              << "              stops dragging its factors; -o DIR also gets robust-weights.sdm, the posterior-mean weight of every training\n"
              << "              cell (one GPU, no -g; not with --weights, --probit, --censored, --noise adaptive, --row-features /\n"
              << "              --col-features, -m / -l, --fp32, --topn-score prob|ei or BPMF_REDUCE=1)\n"
              << "  [--bias] [--bias-lambda F] [--bias-prior A0,B0]: row and column offsets, r = mean + b_row + c_col + u . v with b, c ~ N(0, 1 / F)\n"
              << "              (F = 1 unless given), redrawn on the device in every half-iteration; with --bias-prior F is sampled too, Gamma(A0,\n"
              << "              rate B0) a priori, one per side.  The RMSE columns include the offsets and --topn / --rank-eval rank with them (-d <= 126);\n"
              << "              -o DIR also gets row-bias.ddm and col-bias.ddm (their posterior means, 1 x rows / 1 x cols) and bias_lambda.csv (one\n"
              << "              GPU, no -g; not with another likelihood, --weights, --noise adaptive, features, fold-in, --similar, --save-model /\n"
              << "              --model, -m / -l, --fp32 or BPMF_REDUCE=1)\n"
              << "  [--implicit W0]: implicit feedback: every cell the training matrix does not store is a zero of weight W0 > 0, a stored cell has\n"
              << "              its value and the confidence 1, or its entry of --weights FILE, which must be > W0; mean rating 0; both sides step\n"
              << "              through a blocking half-iteration that forms the Gram matrix of the other side (one GPU, no -g; not with --fp32,\n"
              << "              --probit, --ordinal, --robust, --censored, --noise adaptive, --row-features / --col-features, -m / -l,\n"
              << "              --fold-in-*, --tensor, --topn-score prob|ei or BPMF_REDUCE=1)\n"
              << "  [--rank-eval N]: after the chain rank every held-out test cell among the candidates its query has not rated (1 <= N <= 1000;\n"
              << "              -i > -b, one GPU) and print recall@N, NDCG@N, MRR, the mean percentile rank and the rank AUC; -o DIR also gets\n"
              << "              ranks.csv (query,candidate,rank,ncand)\n"
              << "  [--rank-by rows|cols]: the queries of --rank-eval: rows (users, the default) or columns\n"
              << "  [--rank-threshold F]: the held-out items are the test cells with a value > F (default: every test cell; > 0 under --implicit)\n"
              << "  [--tensor FILE.tns]: factorise a sparse tensor of order 3 (Bayesian CP) instead of a matrix: FILE takes the place of -n / -p;\n"
              << "              FROSTT format, one entry per line, i j t value, 1-based indices, # comments, optional .gz (one GPU, no -g; -i, -b,\n"
              << "              -a, -d and -o apply; not with --fp32, -m / -l, --probit, --censored, --weights, --robust, --noise adaptive,\n"
              << "              features, --topn, fold-in or BPMF_REDUCE=1).  -o DIR gets mode1-mu.ddm .. mode3-mu.ddm, Pavg.tns and Pm2.tns\n"
              << "  [--tensor-test FILE.tns]: held-out entries of the tensor, evaluated after every iteration\n"
              << "  [--tensor-dims I,J,T]: the sizes of the three modes (default: the largest index seen in either file)\n"
              << "  [-t N]: host threads (accepted; the column loop runs on the GPU)\n"
              << "\n"
              << "Matrix formats (by extension, optionally .gz):\n"
              << "  *.mtx / *.mm: MatrixMarket, sparse (coordinate) or dense (array)\n"
              << "  *.sdm / *.sbm: sparse binary double / pattern\n"
              << "  *.ddm / *.csv: dense binary double / text\n"
              << std::endl;
}

// With -g N > 1 the ranks are threads of this process: a rank that fails (Cholesky failed, device wait timed out, a
// collective that gave up) must not run static destructors and the HIP / RCCL teardown under the other ranks' live
// threads -- they may be blocked inside a collective.  Sys::Abort of the reference's MPI back-ends is MPI_Abort
// (c++/mpi_common.h:28-31): the message, then the process ends at once.
std::atomic<bool> g_rank_threads{false};
std::mutex g_die_mutex;
std::vector<std::string> g_rank_files;                               // bpmf_<rank>.out of every rank (-g N / -r): the failure message is appended to each

[[noreturn]] void die(const std::string &msg)
{
    if (g_rank_threads.load()) {
        {   // _Exit runs no destructors.  Every line a rank writes ends in std::endl, so its log file is current up to the line it
            // is formatting right now; the failure message goes into every rank's log through a descriptor of its own (O_APPEND +
            // write): the other ranks' std::ofstream objects are NOT touched from this thread -- they may be inside operator<<
            // (inserting into / flushing them from here was a data race on iostream state that could lose the very
            // diagnostic it was meant to save).
            std::lock_guard<std::mutex> lk(g_die_mutex);
            std::cerr << "bpmf: " << msg << std::endl;
            const std::string line = "bpmf: " + msg + "\n";
            for (const std::string &f : g_rank_files) {
                const int fd = ::open(f.c_str(), O_WRONLY | O_APPEND);
                if (fd >= 0) { ssize_t w = ::write(fd, line.data(), line.size()); (void)w; ::close(fd); }
            }
        }
        std::_Exit(1);
    }
    std::cerr << "bpmf: " << msg << std::endl;
    exit(1);
}

void check(int rc)
{
    if (rc) die(bpmf_hip_last_error());
}

// Sys::init prints (c++/sample.cpp:203-223)
void print_init(std::ostream &os, const char *name, const Csc &M, int64_t test_nnz, double mean_rating)
{
    const int breakpoint1 = 24, breakpoint2 = 10500;        // c++/bpmf.h:255-256
    int64_t bp1 = 0, bp2 = 0;
    for (int64_t k = 0; k < M.ncols; ++k) {
        const int64_t c = M.colptr[(size_t)k + 1] - M.colptr[(size_t)k];
        if (c > breakpoint1) bp1++;
        if (c > breakpoint2) bp2++;
    }
    os << "mean rating: " << mean_rating << std::endl;
    os << "total number of ratings in train: " << M.nnz() << std::endl;
    os << "total number of ratings in test: " << test_nnz << std::endl;
    os << "average ratings per row: " << (double)M.nnz() / (double)M.ncols << std::endl;
    os << "rows > break_point1: " << 100. * (double)bp1 / (double)M.ncols << std::endl;
    os << "rows > break_point2: " << 100. * (double)bp2 / (double)M.ncols << std::endl;
    os << "num " << name << ": " << M.ncols << std::endl;
}

// Contiguous column ranges of equal work, work = c0 + nnz per column -- the reference's assign() balances the same
// quantity with c0 = 10 (c++/assign.cpp:109-120) and then permutes the columns; contiguous cuts of the original
// order keep the column ids, hence the per-column RNG streams and the samples, independent of the GPU count.
// c0: a column costs about as much as 64 ratings here (10M x 1M shard, K = 32: 463 555 columns cost 1.14 ms more
// than 190 with the same 250 M ratings, a rating 0.038 ns: profiles/r01_shard_10Mx1M.txt); BPMF_ASSIGN_COST overrides.
// balance = false (-k): equal column counts, the reference's `!permute` branch (c++/assign.cpp:60-65).
std::vector<int64_t> column_ranges(const Csc &M, int nparts, bool balance)
{
    std::vector<int64_t> b((size_t)nparts + 1, 0);
    const int64_t n = M.ncols;
    if (!balance) {
        const int64_t per = n / nparts;
        for (int p = 0; p < nparts; ++p) b[(size_t)p] = (int64_t)p * per;
        b[(size_t)nparts] = n;
        return b;
    }
    const double c0 = getenv("BPMF_ASSIGN_COST") ? atof(getenv("BPMF_ASSIGN_COST")) : 64.0;
    const double total = (double)M.nnz() + c0 * (double)n;
    int64_t col = 0;
    for (int p = 1; p < nparts; ++p) {
        const double goal = total * p / nparts;
        while (col < n && (double)M.colptr[(size_t)col + 1] + c0 * (double)(col + 1) <= goal) ++col;
        b[(size_t)p] = col;
    }
    b[(size_t)nparts] = n;
    return b;
}

// B = A with its columns renumbered (column j of B = column col_new2old[j] of A) and its row ids mapped through
// row_old2new, rows ascending inside every column again: Sys::permuteCols (c++/assign.cpp:17-36) for both sides at once
Csc permute(const Csc &A, const std::vector<int64_t> &col_new2old, const std::vector<int64_t> &row_old2new)
{
    Csc B;
    B.nrows = A.nrows; B.ncols = A.ncols;
    B.colptr.assign((size_t)A.ncols + 1, 0);
    B.rowidx.resize(A.rowidx.size()); B.vals.resize(A.vals.size());
    std::vector<std::pair<int32_t, double>> tmp;
    int64_t q = 0;
    for (int64_t j = 0; j < A.ncols; ++j) {
        const int64_t o = col_new2old[(size_t)j];
        tmp.clear();
        for (int64_t p = A.colptr[(size_t)o]; p < A.colptr[(size_t)o + 1]; ++p)
            tmp.emplace_back((int32_t)row_old2new[(size_t)A.rowidx[(size_t)p]], A.vals[(size_t)p]);
        std::sort(tmp.begin(), tmp.end(), [](const std::pair<int32_t, double> &a, const std::pair<int32_t, double> &b) { return a.first < b.first; });
        for (auto &e : tmp) { B.rowidx[(size_t)q] = e.first; B.vals[(size_t)q] = e.second; ++q; }
        B.colptr[(size_t)j + 1] = q;
    }
    return B;
}

std::vector<int64_t> inverse(const std::vector<int64_t> &p)
{
    std::vector<int64_t> r(p.size());
    for (size_t i = 0; i < p.size(); ++i) r[(size_t)p[i]] = (int64_t)i;
    return r;
}

// dense K' x N matrix (column-major, one block of `rows` doubles per column): out column j = in column map[j]
void permute_columns(std::vector<double> &d, int64_t rows, const std::vector<int64_t> &map)
{
    if (d.empty()) return;
    std::vector<double> o(d.size());
    for (size_t j = 0; j < map.size(); ++j) memcpy(&o[j * (size_t)rows], &d[(size_t)map[j] * (size_t)rows], sizeof(double) * (size_t)rows);
    d.swap(o);
}

// bpmf_amd.rank_metrics at list length n: rank[p] of held-out entry p among the ncand[q] candidates its query q has not rated, the
// entries of query q at tptr[q] .. tptr[q + 1].  Means over what is named, NaN when that is empty:
//   recall   over the queries with entries: entries with rank <= n / min(n, entries)
//   ndcg     over the same: sum of 1 / log2(1 + rank) over the entries with rank <= n, over sum_{i = 1 .. min(n, entries)} 1 / log2(1 + i)
//   mrr      over the same: 1 / the smallest rank
//   mpr      over the ENTRIES with ncand > 1: (rank - 1) / (ncand - 1)
//   auc      over the queries with entries and other candidates: 1 - sum_i (r_(i) - i) / (entries (ncand - entries)), ranks ascending
struct RankMetrics { double recall = NAN, ndcg = NAN, mrr = NAN, mpr = NAN, auc = NAN; int64_t queries = 0, entries = 0; };
RankMetrics rank_metrics(const std::vector<int32_t> &rank, const std::vector<int64_t> &tptr, const std::vector<int32_t> &ncand, int n)
{
    RankMetrics m;
    double recall = 0.0, ndcg = 0.0, mrr = 0.0, auc = 0.0, mpr = 0.0;
    int64_t nauc = 0, nmpr = 0;
    const int64_t nq = (int64_t)tptr.size() - 1;
    std::vector<int32_t> r;
    for (int64_t q = 0; q < nq; ++q) {
        r.assign(rank.begin() + tptr[(size_t)q], rank.begin() + tptr[(size_t)q + 1]);
        const int64_t h = (int64_t)r.size();
        if (h == 0) continue;
        std::sort(r.begin(), r.end());
        int64_t hits = 0, before = 0;
        double dcg = 0.0, idcg = 0.0;
        for (int64_t i = 0; i < h; ++i) {
            if (r[(size_t)i] <= n) { ++hits; dcg += 1.0 / std::log2(1.0 + (double)r[(size_t)i]); }
            if (i < n) idcg += 1.0 / std::log2(2.0 + (double)i);
            before += (int64_t)r[(size_t)i] - (i + 1);
            if (ncand[(size_t)q] > 1) { mpr += (double)(r[(size_t)i] - 1) / (double)(ncand[(size_t)q] - 1); ++nmpr; }
        }
        recall += (double)hits / (double)std::min<int64_t>(n, h);
        ndcg += dcg / idcg;
        mrr += 1.0 / (double)r[0];
        const int64_t others = (int64_t)ncand[(size_t)q] - h;
        if (others > 0) { auc += 1.0 - (double)before / ((double)h * (double)others); ++nauc; }
        ++m.queries;
        m.entries += h;
    }
    if (m.queries > 0) { m.recall = recall / (double)m.queries; m.ndcg = ndcg / (double)m.queries; m.mrr = mrr / (double)m.queries; }
    if (nmpr > 0) m.mpr = mpr / (double)nmpr;
    if (nauc > 0) m.auc = auc / (double)nauc;
    return m;
}

struct Job {
    // inputs (read-only for the ranks)
    Csc M, Mt, T, Tt;                                                // Tt: the test entries by user (users.predict(movies), c++/bpmf.cpp:190)
    int K = 32, dtype = BPMF_HIP_F64, nsims = 20, burnin = 5, update_freq = 1, nthrds = -1, nranks = 1;
    double alpha = 2.0, mean_m = 0.0, mean_u = 0.0;
    bool verbose = false, redirect = false, sharded = false;
    int topn = 0;                                                    // --topn N (0: off)
    bool topn_by_cols = false;                                       // --topn-by cols: rank the rows (users) of every column (item)
    std::vector<int32_t> topn_idx; std::vector<double> topn_mean, topn_std;   // queries x N, in the numbering of the run
    int topn_kind = -1;                                              // --topn-score: -1 mean, else BPMF_HIP_SCORE_*
    double topn_param = 0.0, topn_sigma = 0.0;                       // kappa or the threshold; the observation noise of prob / ei
    std::vector<double> topn_score;
    int similar = 0;                                                 // --similar N (0: off): the N nearest neighbours of every column (item) or row (user)
    bool similar_by_rows = false;                                    // --similar-by rows
    int similar_kind = BPMF_HIP_SIM_COSINE;                          // --similar-kind cosine|euclid
    double similar_kappa = 0.0;                                      // --similar-kappa F: score = mean - kappa std
    long similar_min = 0;                                            // --similar-min-ratings M: entities with fewer training ratings are not listed
    std::vector<int32_t> sim_idx; std::vector<double> sim_score, sim_mean, sim_std;   // queries x N, in the numbering of the run
    bool diagnose = false;                                           // --diagnose: split-Rhat and ESS of the predictions of a list of cells
    std::vector<int32_t> dg_q, dg_c;                                 // the cells (user, movie), in the numbering of the run
    std::vector<double> dg_mean, dg_std, dg_rhat, dg_ess;            // per cell
    int dg_samples = 0;                                              // the kept samples behind them
    bool diag_rank = false;                                          // --diagnose-rank, or --diagnose under a pooled model: the estimator of DESIGN.md section 33
    int dg_chains = 1;                                               // the chains the rings hold one after the other (--model D0,D1,..)
    std::vector<double> dg_tail;                                     // per cell: the tail ESS (dg_ess is then the bulk ESS, dg_rhat the rank-normalised one)
    int chain = -1;                                                  // --chain c (-1: not given)
    std::vector<double> dg_trace[3];                                 // the post-burn-in traces of RMSE, FU, FM
    double dg_trace_ess[3] = {NAN, NAN, NAN};
    bool score = false;                                              // --score: log predictive density of the test cells, WAIC of the training cells
    struct ScoreSet { bool have = false; std::vector<int32_t> q, c; std::vector<double> y, lpd, pw, mean, std; } sc_test, sc_train;   // cells (user, movie) in the numbering of the run
    std::vector<double> sc_alpha;                                    // the alpha of every kept sample (one value: the same for all)
    int sc_samples = 0;
    bool loo = false;                                                // --loo: PSIS-LOO of the training cells
    std::vector<double> loo_elpd, loo_khat, loo_lpd;                 // per training cell, in the order of M's values
    int loo_samples = 0;
    std::vector<double> iv_levels;                                   // --intervals L1[,L2..]: the levels, as given; the quantile orders they need, increasing
    std::vector<double> iv_tau;
    std::vector<int> iv_lo, iv_hi;                                   // per level: the places of its two ends in iv_tau
    std::vector<int32_t> iv_q, iv_c;                                 // cells (user, movie) in the numbering of the run
    std::vector<double> iv_y, iv_pit, iv_quant, iv_mean, iv_std;     // iv_quant: cells x iv_tau.size()
    int iv_samples = 0;
    bool adaptive = false;                                           // --noise adaptive
    double a0 = 1.0, b0 = 1.0, alpha_max = 0.0;                      // --alpha-prior A0,B0, --alpha-max F (0: no cap)
    std::vector<double> alpha_trace, train_rmse;                     // per iteration: the alpha it ran with, sqrt(SSE / n) after it
    bool probit = false;                                             // --probit
    double probit_threshold = 0.5;                                   // --probit-threshold F
    bool ordinal = false, ord_fixed = false, ord_step_given = false; // --ordinal, --ordinal-cutpoints (fixed), --ordinal-step F
    std::vector<double> ord_levels, ord_cut0;                        // the C level values; the C - 1 initial cutpoints (empty: the library's default)
    double ord_step = 0.0;                                           // the proposal step of the cutpoints (0: 1 / sqrt(nnz), adapted in the burn-in)
    std::vector<double> ord_trace, ord_step_trace, cat_prob;         // per iteration its C - 1 cutpoints and its step; test entries x C probabilities
    std::vector<int> ord_accepted;                                   // per iteration: was its proposal accepted
    double ord_rmse = NAN, ord_accuracy = NAN, ord_logp = NAN;
    bool censored = false;                                           // --censored FILE
    std::vector<int8_t> cens_m, cens_u;                              // the flags of every rating of M / Mt (0, +1 lower bound, -1 upper bound)
    int64_t cens_right = 0, cens_left = 0;
    bool weighted = false;                                           // --weights FILE
    std::vector<double> w_m, w_u;                                    // the weight of every rating of M / Mt
    int64_t w_count = 0; double w_min = 1.0, w_max = 1.0;            // listed cells whose weight is not 1; the smallest / largest weight
    bool robust = false; double robust_nu = 0.0;                     // --robust NU
    bool implicit = false; double implicit_w0 = 0.0;                 // --implicit W0
    bool bias = false; double bias_lambda = 1.0;                     // --bias [--bias-lambda F]
    bool bias_sampled = false; double bias_a0 = 0.0, bias_b0 = 0.0;  // --bias-prior A0,B0
    std::vector<double> bias_lam_u, bias_lam_m;                      // the precision every iteration's step ran with
    std::vector<double> bias_u, bias_m;                              // the posterior-mean bias of every user / movie (the run's numbering)
    int rank_eval = 0;                                               // --rank-eval N (0: off)
    bool rank_by_cols = false, rank_thr_given = false;               // --rank-by cols, --rank-threshold F
    double rank_thr = 0.0;
    std::vector<int64_t> rank_tptr;                                  // per query of the run's numbering: its held-out entries
    std::vector<int32_t> rank_tcand, rank_rank, rank_ncand;          // their candidates (ascending) and ranks; the candidates left per query
    std::vector<double> robust_w;                                    // the posterior-mean weight of every rating of M
    std::vector<double> prob;                                        // posterior-mean probability of a positive, test-set order of T
    double auc = NAN, brier = NAN;
    Dense feat_u, feat_m;                                            // --row-features / --col-features (N x D, column-major; empty: none)
    double lambda_beta = 5.0;                                        // --lambda-beta F
    bool lb_sampled = false; double lb_a0 = 5e-4, lb_b0 = 5e-4;      // --lambda-beta-prior A0,B0: lambda_beta is sampled
    std::vector<double> lb_trace_u, lb_trace_m;                      // the lambda_beta every half-iteration used (-o: DIR/lambda_beta.csv)
    Csc sfeat_u, sfeat_m;                                            // the same from a sparse file: F^T column-compressed = F by rows (D x N)
    int64_t sfeat_u_d = 0, sfeat_m_d = 0;                            // their D (0: none)
    double link_tol = 1e-6; int link_max_iter = 1000;                // --link-tol F / --link-max-iter N (sparse features: the CG draw)
    // --new-row-features / --new-col-features: n x D row-major, or F by rows from a sparse file; n = 0: none
    struct NewRows {
        int64_t n = 0; std::vector<double> F; Csc Fr;
        bool dense_out = true;                                       // the mean / std files fit the cap of 2^28 cells
        std::vector<double> mean, std;                               // new x other side, row-major
        std::vector<int32_t> topn_idx; std::vector<double> topn_mean, topn_std; bool new_are_queries = true;
    } new_u, new_m;
    // --fold-in-rows / --fold-in-cols: Fr holds the RATINGS of the new entities (column i = new entity i, its
    // rows = columns of the other side); n = 0: none
    NewRows fold_u, fold_m;
    bool has_feat_u() const { return !feat_u.data.empty() || sfeat_u_d > 0; }
    bool has_feat_m() const { return !feat_m.data.empty() || sfeat_m_d > 0; }
    std::vector<double> beta_u, beta_m;                              // posterior mean of the link matrices, D x K row-major
    std::string odirname;
    std::string save_model;                                          // --save-model DIR (empty: off)
    Dense prop_m_mu, prop_m_lambda, prop_u_mu, prop_u_lambda;       // -m / -l (empty: none)
    std::vector<int64_t> bm, bu;                                     // column ranges of the ranks
    std::vector<int64_t> perm_m, perm_u;                             // greedy assignment: new column id -> original (empty: none)
    char rccl_id[128];
    std::vector<int> devices;                                        // BPMF_HIP_DEVICES: device of rank r (default: device r)
    // results
    std::vector<double> pavg, pm2;                                   // test-set order of T; every rank fills its slice
    std::vector<double> u_mu, u_lambda, m_mu, m_lambda;              // -o: K x N means, K*K x N precisions; every rank fills its columns
    double elapsed = 0.0, rmse_avg = NAN;
    int64_t num_predict = 0;
    long double average_items_sec = 0, average_ratings_sec = 0;
    std::vector<std::string> errors;                                 // per rank
};

// --topn and --rank-eval over the sample rings of the two sides: after the chain (rank_main) or from a loaded model (run_model)
void serve_rank(Job &J, bpmf_hip_side *users, bpmf_hip_side *movies)
{
    const int64_t nmovies = J.M.ncols, nusers = J.M.nrows;
    if (J.topn > 0) {                                                // one rank (main refuses -g > 1)
        const double t0 = tick();
        bpmf_hip_side *q = J.topn_by_cols ? movies : users, *cand = J.topn_by_cols ? users : movies;
        const int64_t nq = J.topn_by_cols ? nmovies : nusers;
        J.topn_idx.resize((size_t)nq * J.topn); J.topn_mean.resize(J.topn_idx.size()); J.topn_std.resize(J.topn_idx.size());
        if (J.topn_kind < 0) {
            check(bpmf_hip_topn(q, cand, J.mean_m, J.topn, 0, nq, 1, J.topn_idx.data(), J.topn_mean.data(), J.topn_std.data()));
        } else {
            J.topn_score.resize(J.topn_idx.size());
            check(bpmf_hip_topn_scored(q, cand, J.mean_m, J.topn, 0, nq, 1, J.topn_kind, J.topn_param, J.topn_sigma, J.topn_idx.data(),
                                       J.topn_score.data(), J.topn_mean.data(), J.topn_std.data()));
            if (J.topn_kind == BPMF_HIP_SCORE_UCB) std::cerr << "topn score: ucb, kappa = " << J.topn_param << std::endl;
            else std::cerr << "topn score: " << (J.topn_kind == BPMF_HIP_SCORE_PROB ? "prob" : "ei") << ", threshold = " << J.topn_param
                           << ", sigma = " << J.topn_sigma << std::endl;
        }
        std::cerr << "topn: " << J.topn << " per " << (J.topn_by_cols ? "column" : "row") << " for " << nq << " queries, "
                  << (tick() - t0) * 1e3 << " ms" << std::endl;
    }
    if (J.rank_eval > 0) {                                           // one rank (main refuses -g > 1)
        const double t0 = tick();
        bpmf_hip_side *q = J.rank_by_cols ? movies : users, *cand = J.rank_by_cols ? users : movies;
        const int64_t nq = J.rank_by_cols ? nmovies : nusers;
        J.rank_rank.assign(std::max<size_t>(J.rank_tcand.size(), 1), 0); J.rank_ncand.assign((size_t)std::max<int64_t>(nq, 1), 0);
        static const int32_t none = 0;
        check(bpmf_hip_rank_eval(q, cand, J.mean_m, 0, nq, 1, J.rank_tptr.data(), J.rank_tcand.empty() ? &none : J.rank_tcand.data(),
                                 J.rank_rank.data(), J.rank_ncand.data()));
        J.rank_rank.resize(J.rank_tcand.size());
        std::cerr << "rank-eval: " << J.rank_tcand.size() << " held-out entries of " << nq << " queries, " << (tick() - t0) * 1e3 << " ms" << std::endl;
    }
}

// --similar over the sample ring of one side: after the chain or from a loaded model
void serve_similar(Job &J, bpmf_hip_side *users, bpmf_hip_side *movies)
{
    if (J.similar < 1) return;                                       // one rank (main refuses -g > 1)
    const double t0 = tick();
    bpmf_hip_side *side = J.similar_by_rows ? users : movies;
    const Csc &A = J.similar_by_rows ? J.Mt : J.M;                   // one column per entity of the side, in the run's numbering
    const int64_t nq = J.similar_by_rows ? J.M.nrows : J.M.ncols;
    std::vector<uint8_t> ok;
    if (J.similar_min > 0) {
        ok.resize((size_t)std::max<int64_t>(nq, 1));
        for (int64_t c = 0; c < nq; ++c) ok[(size_t)c] = A.colptr[(size_t)c + 1] - A.colptr[(size_t)c] >= (int64_t)J.similar_min ? 1 : 0;
    }
    J.sim_idx.resize((size_t)nq * J.similar); J.sim_score.resize(J.sim_idx.size()); J.sim_mean.resize(J.sim_idx.size()); J.sim_std.resize(J.sim_idx.size());
    check(bpmf_hip_similar(side, J.similar_kind, J.similar_kappa, J.similar, 0, nq, ok.empty() ? nullptr : ok.data(), J.sim_idx.data(),
                           J.sim_score.data(), J.sim_mean.data(), J.sim_std.data()));
    std::cerr << "similar: " << J.similar << " per " << (J.similar_by_rows ? "row" : "column") << " for " << nq << " queries, "
              << (tick() - t0) * 1e3 << " ms" << std::endl;
}

// DIR/similar-cols.csv / similar-rows.csv
void write_similar(const Job &J)
{
    if (J.similar < 1) return;                                       // 1-based ids in the ORIGINAL numbering, like the -o writers
    const std::vector<int64_t> &pq = J.similar_by_rows ? J.perm_u : J.perm_m;
    const int64_t nq = (int64_t)(J.sim_idx.size() / (size_t)J.similar);
    std::vector<int64_t> order((size_t)nq);                          // queries in original order
    for (int64_t i = 0; i < nq; ++i) order[(size_t)i] = i;
    if (!pq.empty()) std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return pq[(size_t)a] < pq[(size_t)b]; });
    const std::string name = J.odirname + (J.similar_by_rows ? "/similar-rows.csv" : "/similar-cols.csv");
    FILE *f = fopen(name.c_str(), "w");
    if (!f) die("cannot write " + name);
    fprintf(f, "# similar %d by %s kind %s kappa %.17g min-ratings %ld\n", J.similar, J.similar_by_rows ? "rows" : "cols",
            J.similar_kind == BPMF_HIP_SIM_COSINE ? "cosine" : "euclid", J.similar_kappa, J.similar_min);
    fprintf(f, "query,rank,neighbour,score,mean,std\n");
    for (int64_t q : order)
        for (int r = 0; r < J.similar; ++r) {
            const size_t at = (size_t)q * J.similar + r;
            const int32_t c = J.sim_idx[at];
            if (c < 0) break;                                        // (padding slots are not written)
            fprintf(f, "%lld,%d,%lld,%.17g,%.17g,%.17g\n", (long long)((pq.empty() ? q : pq[(size_t)q]) + 1), r + 1,
                    (long long)((pq.empty() ? c : pq[(size_t)c]) + 1), J.sim_score[at], J.sim_mean[at], J.sim_std[at]);
        }
    if (fclose(f) != 0) die("cannot write " + name);
}

// --diagnose over the sample rings of both sides: after the chain or from a loaded model, for the cells of
// `cells` (one column per movie) in its order
void serve_diag(Job &J, bpmf_hip_side *users, bpmf_hip_side *movies, const Csc &cells)
{
    if (!J.diagnose) return;                                         // one rank (main refuses -g)
    const double t0 = tick();
    const size_t n = (size_t)cells.nnz();
    J.dg_q.resize(n); J.dg_c.resize(n);
    for (int64_t col = 0; col < cells.ncols; ++col)
        for (int64_t at = cells.colptr[(size_t)col]; at < cells.colptr[(size_t)col + 1]; ++at) {
            J.dg_q[(size_t)at] = cells.rowidx[(size_t)at]; J.dg_c[(size_t)at] = (int32_t)col;
        }
    J.dg_mean.resize(std::max<size_t>(n, 1)); J.dg_std.resize(std::max<size_t>(n, 1)); J.dg_rhat.resize(std::max<size_t>(n, 1)); J.dg_ess.resize(std::max<size_t>(n, 1));
    static const int32_t none = 0;
    if (J.diag_rank) {
        J.dg_tail.resize(std::max<size_t>(n, 1));
        check(bpmf_hip_diag_cells_mc(users, movies, J.mean_m, (int64_t)n, n ? J.dg_q.data() : &none, n ? J.dg_c.data() : &none, J.dg_chains, J.dg_mean.data(),
                                     J.dg_std.data(), J.dg_rhat.data(), J.dg_ess.data(), J.dg_tail.data()));
        J.dg_tail.resize(n);
    } else
    check(bpmf_hip_diag_cells(users, movies, J.mean_m, (int64_t)n, n ? J.dg_q.data() : &none, n ? J.dg_c.data() : &none, J.dg_mean.data(), J.dg_std.data(),
                              J.dg_rhat.data(), J.dg_ess.data()));
    J.dg_mean.resize(n); J.dg_std.resize(n); J.dg_rhat.resize(n); J.dg_ess.resize(n);
    J.dg_samples = bpmf_hip_side_samples_count(users);
    std::cerr << "diagnose: " << n << " cells over " << J.dg_samples << " samples, " << (tick() - t0) * 1e3 << " ms" << std::endl;
}

// DIR/diagnostics.csv: test-set order, 1-based ids in the ORIGINAL numbering, like the -o writers
void write_diag(const Job &J)
{
    if (!J.diagnose || J.odirname.empty()) return;
    const std::string name = J.odirname + "/diagnostics.csv";
    FILE *f = fopen(name.c_str(), "w");
    if (!f) die("cannot write " + name);
    fprintf(f, J.diag_rank ? "row,col,mean,std,rhat,ess_bulk,ess_tail,mcse\n" : "row,col,mean,std,rhat,ess,mcse\n");
    for (size_t i = 0; i < J.dg_q.size(); ++i) {
        const int64_t r = J.dg_q[i], c = J.dg_c[i];
        if (J.diag_rank) {
            fprintf(f, "%lld,%lld,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g\n", (long long)((J.perm_u.empty() ? r : J.perm_u[(size_t)r]) + 1),
                    (long long)((J.perm_m.empty() ? c : J.perm_m[(size_t)c]) + 1), J.dg_mean[i], J.dg_std[i], J.dg_rhat[i], J.dg_ess[i], J.dg_tail[i],
                    J.dg_std[i] / std::sqrt(J.dg_ess[i]));
            continue;
        }
        fprintf(f, "%lld,%lld,%.17g,%.17g,%.17g,%.17g,%.17g\n", (long long)((J.perm_u.empty() ? r : J.perm_u[(size_t)r]) + 1),
                (long long)((J.perm_m.empty() ? c : J.perm_m[(size_t)c]) + 1), J.dg_mean[i], J.dg_std[i], J.dg_rhat[i], J.dg_ess[i],
                J.dg_std[i] / std::sqrt(J.dg_ess[i]));
    }
    if (fclose(f) != 0) die("cannot write " + name);
}

// the Final lines of --diagnose (bpmf_amd.diag_summary computes the same figures): cells whose rhat or ess is NaN are left out
void print_diag(std::ostream &os, const Job &J, bool traces)
{
    if (!J.diagnose) return;
    std::vector<double> rh, es, ms, tl;
    for (size_t i = 0; i < J.dg_rhat.size(); ++i)
        if (!std::isnan(J.dg_rhat[i]) && !std::isnan(J.dg_ess[i]) && !(J.diag_rank && std::isnan(J.dg_tail[i]))) {
            rh.push_back(J.dg_rhat[i]); es.push_back(J.dg_ess[i]); ms.push_back(1.0 / std::sqrt(J.dg_ess[i]));
            if (J.diag_rank) tl.push_back(J.dg_tail[i]);
        }
    auto median = [](std::vector<double> v) {
        if (v.empty()) return (double)NAN;
        std::sort(v.begin(), v.end());
        return v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]);
    };
    size_t above = 0;
    for (double r : rh) above += r > 1.01;
    char buf[512];
    if (J.diag_rank)
        snprintf(buf, sizeof buf, "Final ESS: bulk min %.1f median %.1f tail min %.1f median %.1f of %d samples in %d chains (%lld cells)",
                 es.empty() ? NAN : *std::min_element(es.begin(), es.end()), median(es), tl.empty() ? NAN : *std::min_element(tl.begin(), tl.end()), median(tl),
                 J.dg_samples, J.dg_chains, (long long)J.dg_rhat.size());
    else
    snprintf(buf, sizeof buf, "Final ESS: min %.1f median %.1f of %d samples (%lld cells)", es.empty() ? NAN : *std::min_element(es.begin(), es.end()), median(es),
             J.dg_samples, (long long)J.dg_rhat.size());
    os << buf << std::endl;
    snprintf(buf, sizeof buf, J.diag_rank ? "Final rank-Rhat: median %.4f max %.4f above 1.01: %.2f%%" : "Final split-Rhat: median %.4f max %.4f above 1.01: %.2f%%", median(rh), rh.empty() ? NAN : *std::max_element(rh.begin(), rh.end()),
             rh.empty() ? NAN : 100.0 * (double)above / (double)rh.size());
    os << buf << std::endl;
    snprintf(buf, sizeof buf, "Final MCSE/std: median %.4f", median(ms));
    os << buf << std::endl;
    if (!traces) return;
    snprintf(buf, sizeof buf, "Final trace ESS: RMSE %.1f FU %.1f FM %.1f", J.dg_trace_ess[0], J.dg_trace_ess[1], J.dg_trace_ess[2]);
    os << buf << std::endl;
}

// The cells of `cells` (one column per movie) as the lists a cell query takes -- user, movie and the observed value, in the order of its
// values; probit: the label as +-1 -- resized to at least one entry: what serve_score and serve_loo hand to the library
void observed_cells(const Job &J, const Csc &cells, std::vector<int32_t> &q, std::vector<int32_t> &c, std::vector<double> &y)
{
    const size_t n1 = std::max<size_t>((size_t)cells.nnz(), 1);
    q.resize(n1); c.resize(n1); y.resize(n1);
    for (int64_t col = 0; col < cells.ncols; ++col)
        for (int64_t at = cells.colptr[(size_t)col]; at < cells.colptr[(size_t)col + 1]; ++at) {
            q[(size_t)at] = cells.rowidx[(size_t)at]; c[(size_t)at] = (int32_t)col;
            y[(size_t)at] = J.probit ? (cells.vals[(size_t)at] > J.probit_threshold ? 1.0 : -1.0) : cells.vals[(size_t)at];
        }
}

// --score over the sample rings of both sides: after the chain or from a loaded model.  `test` (NULL: none): the
// held-out cells with their values; `train` (NULL: none): the training cells, with the weights and censoring flags of the run.  The
// likelihood is the run's: probit, Student-t under --robust, else Gaussian; J.sc_alpha holds the alpha of the kept samples.
void serve_score(Job &J, bpmf_hip_side *users, bpmf_hip_side *movies, const Csc *test, const Csc *train)
{
    if (!J.score) return;                                            // one rank (main refuses -g)
    const double t0 = tick();
    const int kind = J.probit ? BPMF_HIP_LOGDENS_PROBIT : J.robust ? BPMF_HIP_LOGDENS_STUDENT : BPMF_HIP_LOGDENS_GAUSSIAN;
    auto run = [&](const Csc &cells, Job::ScoreSet &out, const double *w, const int8_t *flag) {
        const size_t n = (size_t)cells.nnz(), n1 = std::max<size_t>(n, 1);
        out.have = true;
        observed_cells(J, cells, out.q, out.c, out.y);
        out.lpd.resize(n1); out.pw.resize(n1); out.mean.resize(n1); out.std.resize(n1);
        check(bpmf_hip_score_cells(users, movies, J.mean_m, (int64_t)n, out.q.data(), out.c.data(), out.y.data(), n ? w : nullptr, n ? flag : nullptr, kind,
                                   J.robust_nu, (int)J.sc_alpha.size(), J.sc_alpha.data(), out.lpd.data(), out.pw.data(), out.mean.data(), out.std.data()));
        out.q.resize(n); out.c.resize(n); out.y.resize(n); out.lpd.resize(n); out.pw.resize(n); out.mean.resize(n); out.std.resize(n);
    };
    if (test) run(*test, J.sc_test, nullptr, nullptr);
    if (train) run(*train, J.sc_train, J.weighted && !J.implicit ? J.w_m.data() : nullptr, J.censored ? J.cens_m.data() : nullptr);
    J.sc_samples = bpmf_hip_side_samples_count(users);
    std::cerr << "score: " << (test ? J.sc_test.q.size() : 0) << " test and " << (train ? J.sc_train.q.size() : 0) << " training cells over " << J.sc_samples
              << " samples, " << (tick() - t0) * 1e3 << " ms" << std::endl;
}

// DIR/score.csv: the test cells in test-set order, 1-based ids in the ORIGINAL numbering, with the value as given; DIR/waic-elpd.sdm:
// lpd - var of every training cell in the training matrix's original numbering (like robust-weights.sdm)
void write_score(const Job &J, const Csc *test, const Csc *train)
{
    if (!J.score || J.odirname.empty()) return;
    if (J.sc_test.have && test) {
        const std::string name = J.odirname + "/score.csv";
        FILE *f = fopen(name.c_str(), "w");
        if (!f) die("cannot write " + name);
        fprintf(f, "row,col,value,lpd,mean,std\n");
        for (size_t i = 0; i < J.sc_test.q.size(); ++i) {
            const int64_t r = J.sc_test.q[i], c = J.sc_test.c[i];
            fprintf(f, "%lld,%lld,%.17g,%.17g,%.17g,%.17g\n", (long long)((J.perm_u.empty() ? r : J.perm_u[(size_t)r]) + 1),
                    (long long)((J.perm_m.empty() ? c : J.perm_m[(size_t)c]) + 1), test->vals[i], J.sc_test.lpd[i], J.sc_test.mean[i], J.sc_test.std[i]);
        }
        if (fclose(f) != 0) die("cannot write " + name);
    }
    if (J.sc_train.have && train && !J.sc_train.q.empty()) {
        try {
            Csc P = *train;
            for (size_t i = 0; i < P.vals.size(); ++i) P.vals[i] = J.sc_train.lpd[i] - J.sc_train.pw[i];
            if (!J.perm_m.empty()) P = permute(P, inverse(J.perm_m), J.perm_u);
            bpmf::io::write_sparse(J.odirname + "/waic-elpd.sdm", P);
        } catch (const std::exception &e) { die(e.what()); }
    }
}

// the Final lines of --score (bpmf_amd.score_summary computes the same figures)
void print_score(std::ostream &os, const Job &J)
{
    if (!J.score) return;
    auto sum_se = [](const std::vector<double> &x, double *sum, double *se) {      // the sum and sqrt(n var), var with n - 1
        const size_t n = x.size();
        double s = 0.0, v = 0.0;
        for (double e : x) s += e;
        const double m = n ? s / (double)n : 0.0;
        for (double e : x) v += (e - m) * (e - m);
        *sum = s; *se = n > 1 ? std::sqrt((double)n * (v / (double)(n - 1))) : 0.0;
    };
    char buf[512];
    if (J.sc_test.have) {
        double s, se;
        sum_se(J.sc_test.lpd, &s, &se);
        const double n = (double)J.sc_test.lpd.size();
        snprintf(buf, sizeof buf, "Final test log-density: mean %.6f se %.6f (%lld cells, %d samples)", n > 0 ? s / n : NAN, n > 0 ? se / n : NAN,
                 (long long)J.sc_test.lpd.size(), J.sc_samples);
        os << buf << std::endl;
    }
    if (J.sc_train.have) {
        std::vector<double> e(J.sc_train.lpd.size());
        double pw = 0.0; size_t above = 0;
        for (size_t i = 0; i < e.size(); ++i) { e[i] = J.sc_train.lpd[i] - J.sc_train.pw[i]; pw += J.sc_train.pw[i]; above += J.sc_train.pw[i] > 0.4; }
        double s, se;
        sum_se(e, &s, &se);
        snprintf(buf, sizeof buf, "Final WAIC: %.4f elpd %.4f p_waic %.4f se %.4f (%lld cells, %.2f%% with var > 0.4)", -2.0 * s, s, pw, se, (long long)e.size(),
                 e.empty() ? NAN : 100.0 * (double)above / (double)e.size());
        os << buf << std::endl;
    }
}

// --loo over the sample rings of both sides: after the chain or from a loaded model, for the training cells with the
// weights and censoring flags of the run, under the likelihood serve_score names; J.sc_alpha holds the alpha of the kept samples.
void serve_loo(Job &J, bpmf_hip_side *users, bpmf_hip_side *movies, const Csc &train)
{
    if (!J.loo) return;                                              // one rank (main refuses -g)
    const double t0 = tick();
    const int kind = J.probit ? BPMF_HIP_LOGDENS_PROBIT : J.robust ? BPMF_HIP_LOGDENS_STUDENT : BPMF_HIP_LOGDENS_GAUSSIAN;
    const size_t n = (size_t)train.nnz(), n1 = std::max<size_t>(n, 1);
    std::vector<int32_t> q, c;
    std::vector<double> y;
    observed_cells(J, train, q, c, y);
    J.loo_elpd.resize(n1); J.loo_khat.resize(n1); J.loo_lpd.resize(n1);
    check(bpmf_hip_loo_cells(users, movies, J.mean_m, (int64_t)n, q.data(), c.data(), y.data(), n && J.weighted && !J.implicit ? J.w_m.data() : nullptr,
                             n && J.censored ? J.cens_m.data() : nullptr, kind, J.robust_nu, (int)J.sc_alpha.size(), J.sc_alpha.data(), J.loo_elpd.data(),
                             J.loo_khat.data(), J.loo_lpd.data(), nullptr, nullptr));
    J.loo_elpd.resize(n); J.loo_khat.resize(n); J.loo_lpd.resize(n);
    J.loo_samples = bpmf_hip_side_samples_count(users);
    std::cerr << "loo: " << n << " training cells over " << J.loo_samples << " samples, " << (tick() - t0) * 1e3 << " ms" << std::endl;
}

// DIR/loo-elpd.sdm and DIR/loo-khat.sdm: elpd_loo and khat of every training cell in the training matrix's original numbering (like
// waic-elpd.sdm); an infinite khat is written as inf
void write_loo(const Job &J, const Csc &train)
{
    if (!J.loo || J.odirname.empty() || J.loo_elpd.empty()) return;
    try {
        for (int which = 0; which < 2; ++which) {
            Csc P = train;
            P.vals = which ? J.loo_khat : J.loo_elpd;
            if (!J.perm_m.empty()) P = permute(P, inverse(J.perm_m), J.perm_u);
            bpmf::io::write_sparse(J.odirname + (which ? "/loo-khat.sdm" : "/loo-elpd.sdm"), P);
        }
    } catch (const std::exception &e) { die(e.what()); }
}

// the Final line of --loo (bpmf_amd.loo_summary computes the same figures)
void print_loo(std::ostream &os, const Job &J)
{
    if (!J.loo) return;
    const size_t n = J.loo_elpd.size();
    double s = 0.0, v = 0.0, p = 0.0;
    size_t above = 0;
    for (size_t i = 0; i < n; ++i) { s += J.loo_elpd[i]; p += J.loo_lpd[i] - J.loo_elpd[i]; above += J.loo_khat[i] > 0.7; }
    const double m = n ? s / (double)n : 0.0;
    for (double e : J.loo_elpd) v += (e - m) * (e - m);
    const double se = n > 1 ? std::sqrt((double)n * (v / (double)(n - 1))) : 0.0;
    char buf[512];
    snprintf(buf, sizeof buf, "Final PSIS-LOO: looic %.4f elpd %.4f p_loo %.4f se %.4f (%lld cells, %d samples, %.2f%% with k > 0.7)", -2.0 * s, s, p, se,
             (long long)n, J.loo_samples, n ? 100.0 * (double)above / (double)n : NAN);
    os << buf << std::endl;
}

// --intervals over the sample rings of both sides: after the chain or from a loaded model, for the cells of `cells`
// (one column per movie) with their values as the observations, weight 1; J.sc_alpha holds the alpha of the kept samples.
void serve_intervals(Job &J, bpmf_hip_side *users, bpmf_hip_side *movies, const Csc &cells)
{
    if (J.iv_levels.empty()) return;                                 // one rank (main refuses -g)
    const double t0 = tick();
    const size_t n = (size_t)cells.nnz(), n1 = std::max<size_t>(n, 1), nq = J.iv_tau.size();
    J.iv_q.resize(n1); J.iv_c.resize(n1); J.iv_y.resize(n1); J.iv_pit.resize(n1); J.iv_quant.resize(n1 * nq); J.iv_mean.resize(n1); J.iv_std.resize(n1);
    for (int64_t col = 0; col < cells.ncols; ++col)
        for (int64_t at = cells.colptr[(size_t)col]; at < cells.colptr[(size_t)col + 1]; ++at) {
            J.iv_q[(size_t)at] = cells.rowidx[(size_t)at]; J.iv_c[(size_t)at] = (int32_t)col; J.iv_y[(size_t)at] = cells.vals[(size_t)at];
        }
    check(bpmf_hip_interval_cells(users, movies, J.mean_m, (int64_t)n, J.iv_q.data(), J.iv_c.data(), J.iv_y.data(), nullptr, (int)J.sc_alpha.size(),
                                  J.sc_alpha.data(), (int)nq, J.iv_tau.data(), J.iv_pit.data(), J.iv_quant.data(), J.iv_mean.data(), J.iv_std.data()));
    J.iv_q.resize(n); J.iv_c.resize(n); J.iv_y.resize(n); J.iv_pit.resize(n); J.iv_quant.resize(n * nq); J.iv_mean.resize(n); J.iv_std.resize(n);
    J.iv_samples = bpmf_hip_side_samples_count(users);
    std::cerr << "intervals: " << n << " cells over " << J.iv_samples << " samples, " << (tick() - t0) * 1e3 << " ms" << std::endl;
}

// the level as the column names of intervals.csv and the Final line carry it: its percentage in the shortest form (90, 99.8)
std::string level_name(double level)
{
    char buf[64];
    snprintf(buf, sizeof buf, "%.10g", 100.0 * level);
    return buf;
}

// DIR/intervals.csv: the cells in test-set order, 1-based ids in the ORIGINAL numbering, with the value as given
void write_intervals(const Job &J)
{
    if (J.iv_levels.empty() || J.odirname.empty()) return;
    const std::string name = J.odirname + "/intervals.csv";
    FILE *f = fopen(name.c_str(), "w");
    if (!f) die("cannot write " + name);
    fprintf(f, "row,col,value,mean,std,pit");
    for (double l : J.iv_levels) fprintf(f, ",lo%s,hi%s", level_name(l).c_str(), level_name(l).c_str());
    fprintf(f, "\n");
    const size_t nq = J.iv_tau.size();
    for (size_t i = 0; i < J.iv_q.size(); ++i) {
        const int64_t r = J.iv_q[i], c = J.iv_c[i];
        fprintf(f, "%lld,%lld,%.17g,%.17g,%.17g,%.17g", (long long)((J.perm_u.empty() ? r : J.perm_u[(size_t)r]) + 1),
                (long long)((J.perm_m.empty() ? c : J.perm_m[(size_t)c]) + 1), J.iv_y[i], J.iv_mean[i], J.iv_std[i], J.iv_pit[i]);
        for (size_t k = 0; k < J.iv_levels.size(); ++k) fprintf(f, ",%.17g,%.17g", J.iv_quant[i * nq + (size_t)J.iv_lo[k]], J.iv_quant[i * nq + (size_t)J.iv_hi[k]]);
        fprintf(f, "\n");
    }
    if (fclose(f) != 0) die("cannot write " + name);
}

// the Final lines of --intervals (bpmf_amd.calibration_summary computes the same figures): cells whose pit is NaN are left out
void print_intervals(std::ostream &os, const Job &J)
{
    if (J.iv_levels.empty()) return;
    const size_t nq = J.iv_tau.size();
    std::vector<double> p;
    std::vector<size_t> at;
    for (size_t i = 0; i < J.iv_pit.size(); ++i) if (!std::isnan(J.iv_pit[i])) { p.push_back(J.iv_pit[i]); at.push_back(i); }
    const double n = (double)p.size();
    std::string line = "Final coverage:";
    char buf[256];
    for (size_t k = 0; k < J.iv_levels.size(); ++k) {
        const double l = J.iv_levels[k];
        size_t inside = 0;
        double width = 0.0;
        for (size_t j = 0; j < p.size(); ++j) {
            inside += std::fabs(p[j] - 0.5) <= 0.5 * l;
            width += J.iv_quant[at[j] * nq + (size_t)J.iv_hi[k]] - J.iv_quant[at[j] * nq + (size_t)J.iv_lo[k]];
        }
        snprintf(buf, sizeof buf, " %s%%: %.3f (se %.3f, width %.2f)", level_name(l).c_str(), p.empty() ? NAN : (double)inside / n,
                 p.empty() ? NAN : std::sqrt(l * (1.0 - l) / n), p.empty() ? NAN : width / n);
        line += buf;
    }
    snprintf(buf, sizeof buf, " (%lld cells, %d samples)", (long long)p.size(), J.iv_samples);
    os << line << buf << std::endl;
    std::sort(p.begin(), p.end());
    double ks = p.empty() ? NAN : 0.0;
    for (size_t i = 0; i < p.size(); ++i) ks = std::max(ks, std::max((double)(i + 1) / n - p[i], p[i] - (double)i / n));
    snprintf(buf, sizeof buf, "Final PIT: KS %.3f", ks);
    os << buf << std::endl;
}

// --fold-in-rows / --fold-in-cols against the sample ring of the other side and the side's hyper ring: after the chain or from a loaded model
void serve_fold(Job &J, bpmf_hip_side *users, bpmf_hip_side *movies)
{
    const int64_t nmovies = J.M.ncols, nusers = J.M.nrows;
    // fold-in (streams: tag 7 = new users, 8 = new movies): one launch over every (new entity, kept sample), then the block and the lists
    auto fold_in = [&](bpmf_hip_side *side, bpmf_hip_side *cand, Job::NewRows &N, int64_t nc, unsigned tag) {
        if (N.n == 0) return;
        const double t0 = tick();
        static const int32_t none = 0; static const double zero = 0.0;
        check(bpmf_hip_foldin(side, cand, J.mean_m, N.n, N.Fr.colptr.data(), N.Fr.rowidx.empty() ? &none : N.Fr.rowidx.data(),
                              N.Fr.vals.empty() ? &zero : N.Fr.vals.data(), tag, 1));
        if (N.dense_out) {
            N.mean.resize((size_t)N.n * (size_t)nc); N.std.resize(N.mean.size());
            const int64_t step = std::max<int64_t>(64, ((int64_t)1 << 24) / std::max<int64_t>(nc, 1) / 64 * 64);
            for (int64_t q0 = 0; q0 < N.n; q0 += step) {
                const int64_t q1 = std::min(N.n, q0 + step);
                check(bpmf_hip_foldin_predict(side, cand, J.mean_m, q0, q1, 0, nc, N.mean.data() + (size_t)q0 * nc, N.std.data() + (size_t)q0 * nc));
            }
        }
        if (J.topn > 0) {
            N.new_are_queries = true;
            N.topn_idx.resize((size_t)N.n * J.topn); N.topn_mean.resize(N.topn_idx.size()); N.topn_std.resize(N.topn_idx.size());
            check(bpmf_hip_foldin_topn(side, cand, J.mean_m, J.topn, 1, N.topn_idx.data(), N.topn_mean.data(), N.topn_std.data()));
        }
        std::cerr << "fold-in " << (side == users ? "rows" : "columns") << ": " << N.n << " x " << nc << " predictions, " << (tick() - t0) * 1e3 << " ms" << std::endl;
    };
    fold_in(users, movies, J.fold_u, nmovies, 7);
    fold_in(movies, users, J.fold_m, nusers, 8);
}

// DIR/topn.csv
void write_topn(const Job &J)
{
    if (J.topn > 0) {                                                // 1-based ids in the ORIGINAL numbering, like the -o writers
        const std::vector<int64_t> &pq = J.topn_by_cols ? J.perm_m : J.perm_u, &pc = J.topn_by_cols ? J.perm_u : J.perm_m;
        const int64_t nq = (int64_t)(J.topn_idx.size() / (size_t)J.topn);
        std::vector<int64_t> order((size_t)nq);                      // queries in original order
        for (int64_t i = 0; i < nq; ++i) order[(size_t)i] = i;
        if (!pq.empty()) std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return pq[(size_t)a] < pq[(size_t)b]; });
        FILE *f = fopen((J.odirname + "/topn.csv").c_str(), "w");
        if (!f) die("cannot write " + J.odirname + "/topn.csv");
        fprintf(f, J.topn_kind < 0 ? "query,rank,candidate,mean,std\n" : "query,rank,candidate,score,mean,std\n");
        for (int64_t q : order)
            for (int r = 0; r < J.topn; ++r) {
                const size_t at = (size_t)q * J.topn + r;
                const int32_t c = J.topn_idx[at];
                if (c < 0) break;                                      // (padding slots are not written)
                const long long qid = (long long)((pq.empty() ? q : pq[(size_t)q]) + 1), cid = (long long)((pc.empty() ? c : pc[(size_t)c]) + 1);
                if (J.topn_kind < 0) fprintf(f, "%lld,%d,%lld,%.17g,%.17g\n", qid, r + 1, cid, J.topn_mean[at], J.topn_std[at]);
                else fprintf(f, "%lld,%d,%lld,%.17g,%.17g,%.17g\n", qid, r + 1, cid, J.topn_score[at], J.topn_mean[at], J.topn_std[at]);
            }
        if (fclose(f) != 0) die("cannot write " + J.odirname + "/topn.csv");
    }
}

// --rank-eval: the metrics (the arithmetic of bpmf_amd.rank_metrics), and with -o DIR the rank of every held-out entry in DIR/ranks.csv
RankMetrics write_ranks(const Job &J)
{
    RankMetrics rkm;
    if (J.rank_eval > 0) {
        rkm = rank_metrics(J.rank_rank, J.rank_tptr, J.rank_ncand, J.rank_eval);
        if (!J.odirname.empty()) {                                   // 1-based ids in the ORIGINAL numbering, the queries in their order
            const std::vector<int64_t> &pq = J.rank_by_cols ? J.perm_m : J.perm_u, &pc = J.rank_by_cols ? J.perm_u : J.perm_m;
            const int64_t nq = (int64_t)J.rank_tptr.size() - 1;
            std::vector<int64_t> order((size_t)nq);
            for (int64_t i = 0; i < nq; ++i) order[(size_t)i] = i;
            if (!pq.empty()) std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return pq[(size_t)a] < pq[(size_t)b]; });
            FILE *f = fopen((J.odirname + "/ranks.csv").c_str(), "w");
            if (!f) die("cannot write " + J.odirname + "/ranks.csv");
            fprintf(f, "query,candidate,rank,ncand\n");
            for (int64_t q : order)
                for (int64_t p = J.rank_tptr[(size_t)q]; p < J.rank_tptr[(size_t)q + 1]; ++p) {
                    const int32_t c = J.rank_tcand[(size_t)p];
                    fprintf(f, "%lld,%lld,%d,%d\n", (long long)((pq.empty() ? q : pq[(size_t)q]) + 1), (long long)((pc.empty() ? c : pc[(size_t)c]) + 1),
                            J.rank_rank[(size_t)p], J.rank_ncand[(size_t)q]);
                }
            if (fclose(f) != 0) die("cannot write " + J.odirname + "/ranks.csv");
        }
    }
    return rkm;
}

// the new entities: new x movies as it is computed; users x new = the transpose of what is computed (row-major new x users IS
// column-major users x new).  Lists: 1-based ids, the new entities numbered by their row in the feature file.
void write_new(const Job &J, Job::NewRows &N, bool rows, int64_t nother, const char *stem)
{
    if (N.n == 0) return;
    const std::string base = J.odirname + "/" + stem + (rows ? "-rows" : "-cols");
    try {
        if (N.dense_out) {
            for (int which = 0; which < 2; ++which) {
                std::vector<double> &src = which ? N.std : N.mean;
                Dense d;
                if (rows) {                                        // row-major new x movies -> column-major
                    d.nrows = N.n; d.ncols = nother; d.data.resize(src.size());
                    for (int64_t i = 0; i < N.n; ++i)
                        for (int64_t c = 0; c < nother; ++c) d.data[(size_t)c * (size_t)N.n + (size_t)i] = src[(size_t)i * (size_t)nother + (size_t)c];
                } else { d.nrows = nother; d.ncols = N.n; d.data.swap(src); }
                bpmf::io::write_dense(base + (which ? "-std.ddm" : "-mean.ddm"), d);
            }
        }
    } catch (const std::exception &e) { die(e.what()); }
    if (J.topn > 0) {
        const std::string name = base + "-topn.csv";
        FILE *f = fopen(name.c_str(), "w");
        if (!f) die("cannot write " + name);
        fprintf(f, "query,rank,candidate,mean,std\n");
        const int64_t nq = (int64_t)(N.topn_idx.size() / (size_t)J.topn);
        for (int64_t q = 0; q < nq; ++q)
            for (int r = 0; r < J.topn; ++r) {
                const size_t at = (size_t)q * J.topn + r;
                if (N.topn_idx[at] < 0) break;                     // (padding slots are not written)
                fprintf(f, "%lld,%d,%lld,%.17g,%.17g\n", (long long)(q + 1), r + 1, (long long)(N.topn_idx[at] + 1), N.topn_mean[at], N.topn_std[at]);
            }
        if (fclose(f) != 0) die("cannot write " + name);
    }
}

// the ratings of the entities to fold in: new users x movies / users x new movies; every cell once, finite; stored by new entity
void read_fold(const Job &J, const std::string &name, bool rows, Job::NewRows &N)
{
    if (name.empty()) return;
    const int64_t nmovies = J.M.ncols, nusers = J.M.nrows;
    const std::string w = rows ? "--fold-in-rows" : "--fold-in-cols";
    const int64_t nother = rows ? nmovies : nusers;
    Csc F;
    try { F = bpmf::io::read_sparse(name); } catch (const std::exception &e) { die(e.what()); }
    if ((rows ? F.ncols : F.nrows) != nother)
        die(w + ": " + name + " is " + std::to_string(F.nrows) + " x " + std::to_string(F.ncols) + ", the training matrix has " + std::to_string(nother) +
            (rows ? " columns" : " rows"));
    const int64_t n = rows ? F.nrows : F.ncols;
    if (n < 1) die(w + ": " + name + (rows ? " has no rows" : " has no columns"));
    if (F.dup_row >= 0)
        die(w + ": " + name + " lists cell (" + std::to_string((long long)F.dup_row + 1) + ", " + std::to_string((long long)F.dup_col + 1) + ") twice");
    for (double v : F.vals) if (!std::isfinite(v)) die(w + ": " + name + " holds a value that is not finite");
    N.n = n;
    if (n > ((int64_t)1 << 28) / std::max<int64_t>(nother, 1)) {
        const std::string cells = std::to_string(n) + " x " + std::to_string(nother) + " predictions are more than 2^28 cells per file";
        if (J.topn < 1) die(w + ": " + cells + ": ask for the best N of every query with --topn N instead");
        std::cerr << w << ": " << cells << ": the dense mean / std files are skipped, the --topn lists are written" << std::endl;
        N.dense_out = false;
    }
    N.Fr = rows ? bpmf::io::transpose(F) : F;                     // column i = new entity i, its row ids ascending
}

// --rank-eval: the held-out candidates of every query from the test matrix, ascending (the run's numbering)
void build_rank_lists(Job &J)
{
    if (J.rank_eval > 0) {                                           // the held-out candidates of every query, ascending (the run's numbering)
        const Csc &Q = J.rank_by_cols ? J.T : J.Tt;                  // one column per query
        J.rank_tptr.assign((size_t)Q.ncols + 1, 0);
        for (int64_t q = 0; q < Q.ncols; ++q) {
            std::vector<int32_t> c;
            for (int64_t p = Q.colptr[(size_t)q]; p < Q.colptr[(size_t)q + 1]; ++p)
                if (!J.rank_thr_given || Q.vals[(size_t)p] > J.rank_thr) c.push_back(Q.rowidx[(size_t)p]);
            std::sort(c.begin(), c.end());
            J.rank_tcand.insert(J.rank_tcand.end(), c.begin(), c.end());
            J.rank_tptr[(size_t)q + 1] = (int64_t)J.rank_tcand.size();
        }
    }
}

// one rank = one GPU: Sys::Sys + init (its shard), the Gibbs loop of c++/bpmf.cpp:180-253
void rank_main(Job &J, int rank, std::ostream &os)
{
    const int K = J.K;
    const int64_t nmovies = J.M.ncols, nusers = J.M.nrows;
    const bool aggregate = !J.odirname.empty();
    bpmf_hip_ctx *ctx = nullptr;
    check(bpmf_hip_ctx_create_ex(J.devices.empty() ? rank : J.devices[(size_t)rank % J.devices.size()], K, J.dtype, nullptr, &ctx));
    if (J.sharded) check(bpmf_hip_ctx_comm_init(ctx, J.nranks, rank, J.rccl_id));
    const int64_t m0 = J.bm[(size_t)rank], m1 = J.bm[(size_t)rank + 1], u0 = J.bu[(size_t)rank], u1 = J.bu[(size_t)rank + 1];
    auto slice_ptr = [](const Csc &A, int64_t c0, int64_t c1) {       // colptr of the columns [c0, c1), rebased to 0
        std::vector<int64_t> cp((size_t)(c1 - c0) + 1);
        for (int64_t c = c0; c <= c1; ++c) cp[(size_t)(c - c0)] = A.colptr[(size_t)c] - A.colptr[(size_t)c0];
        return cp;
    };
    bpmf_hip_side *movies = nullptr, *users = nullptr;
    bpmf_hip_test *test = nullptr, *test_u = nullptr;
    {
        const std::vector<int64_t> cp = slice_ptr(J.M, m0, m1);
        const size_t off = (size_t)J.M.colptr[(size_t)m0];
        check(bpmf_hip_side_create(ctx, nmovies, nusers, m0, m1, cp.data(), J.M.rowidx.data() + off, J.M.vals.data() + off, J.mean_m, &movies));
    }
    print_init(os, "movs", J.M, J.T.nnz(), J.mean_m);
    {
        const std::vector<int64_t> cp = slice_ptr(J.Mt, u0, u1);
        const size_t off = (size_t)J.Mt.colptr[(size_t)u0];
        check(bpmf_hip_side_create(ctx, nusers, nmovies, u0, u1, cp.data(), J.Mt.rowidx.data() + off, J.Mt.vals.data() + off, J.mean_u, &users));
    }
    if (J.chain >= 0) {                                              // --chain c: both sides, before their first half-iteration
        check(bpmf_hip_side_set_chain(movies, J.chain));
        check(bpmf_hip_side_set_chain(users, J.chain));
    }
    if (J.probit) {                                                  // (streams: tag 1 = movies, 2 = users)
        check(bpmf_hip_side_set_probit(movies, J.probit_threshold, 1));
        check(bpmf_hip_side_set_probit(users, J.probit_threshold, 2));
    }
    if (J.ordinal) {                                                 // (streams: tag 11 = movies, 12 = users); both sides hold the same cutpoints
        const int C = (int)J.ord_levels.size();
        check(bpmf_hip_side_set_ordinal(movies, J.ord_levels.data(), C, J.ord_fixed ? J.ord_cut0.data() : nullptr, 11));
        J.ord_cut0.resize((size_t)C - 1);
        check(bpmf_hip_side_ordinal_cut_get(movies, J.ord_cut0.data()));
        check(bpmf_hip_side_set_ordinal(users, J.ord_levels.data(), C, J.ord_cut0.data(), 12));
    }
    if (J.censored) {                                                // (streams: tag 5 = movies, 6 = users)
        check(bpmf_hip_side_set_censored(movies, J.cens_m.data(), 5));
        check(bpmf_hip_side_set_censored(users, J.cens_u.data(), 6));
    }
    if (J.implicit) {                                                // (--weights FILE: the confidences)
        check(bpmf_hip_side_set_implicit(movies, J.implicit_w0, J.weighted ? J.w_m.data() : nullptr));
        check(bpmf_hip_side_set_implicit(users, J.implicit_w0, J.weighted ? J.w_u.data() : nullptr));
    } else if (J.weighted) {
        check(bpmf_hip_side_set_weights(movies, J.w_m.data()));
        check(bpmf_hip_side_set_weights(users, J.w_u.data()));
    }
    if (J.bias) {                                            // (streams: tag 13 = movies, 14 = users; roles 0 / 1)
        check(bpmf_hip_side_set_bias(movies, J.bias_lambda, 13, 0));
        check(bpmf_hip_side_set_bias(users, J.bias_lambda, 14, 1));
        if (J.bias_sampled) { check(bpmf_hip_side_bias_prior(movies, J.bias_a0, J.bias_b0)); check(bpmf_hip_side_bias_prior(users, J.bias_a0, J.bias_b0)); }
    }
    if (J.robust) {                                          // (streams: tag 9 = movies, 10 = users; 7 and 8 are the fold-in's)
        check(bpmf_hip_side_set_robust(movies, J.robust_nu, 9));
        check(bpmf_hip_side_set_robust(users, J.robust_nu, 10));
    }
    const bool linked = J.has_feat_u() || J.has_feat_m();   // (streams: tag 3 = movies, 4 = users)
    auto set_sparse = [&](bpmf_hip_side *side, const Csc &Fr, int64_t D, unsigned tag) {       // Fr: F by rows (column = item)
        bool ones = true;
        for (double v : Fr.vals) if (v != 1.0) { ones = false; break; }
        static const int32_t none = 0;
        check(bpmf_hip_side_set_features_sparse(side, (int)D, Fr.colptr.data(), Fr.rowidx.empty() ? &none : Fr.rowidx.data(),
                                                ones ? nullptr : Fr.vals.data(), J.lambda_beta, tag));
        check(bpmf_hip_side_link_cg_set(side, J.link_tol, J.link_max_iter));
    };
    if (J.sfeat_m_d > 0) set_sparse(movies, J.sfeat_m, J.sfeat_m_d, 3);
    else if (J.has_feat_m()) check(bpmf_hip_side_set_features(movies, J.feat_m.data.data(), (int)J.feat_m.ncols, 0, J.lambda_beta, 3));
    if (J.sfeat_u_d > 0) set_sparse(users, J.sfeat_u, J.sfeat_u_d, 4);
    else if (J.has_feat_u()) check(bpmf_hip_side_set_features(users, J.feat_u.data.data(), (int)J.feat_u.ncols, 0, J.lambda_beta, 4));
    if (J.lb_sampled) {
        if (J.has_feat_m()) check(bpmf_hip_side_link_lambda_prior(movies, J.lb_a0, J.lb_b0));
        if (J.has_feat_u()) check(bpmf_hip_side_link_lambda_prior(users, J.lb_a0, J.lb_b0));
    }
    // a ring of the post-burn-in samples of a side: --topn, or the candidates of the other side's new entities
    const bool saving = !J.save_model.empty();
    const bool ring_m = J.topn > 0 || J.new_u.n > 0 || J.fold_u.n > 0 || J.rank_eval > 0 || saving || (J.similar > 0 && !J.similar_by_rows) || J.diagnose || J.score || !J.iv_levels.empty() || J.loo, ring_u = J.topn > 0 || J.new_m.n > 0 || J.fold_m.n > 0 || J.rank_eval > 0 || saving || (J.similar > 0 && J.similar_by_rows) || J.diagnose || J.score || !J.iv_levels.empty() || J.loo;
    if (ring_m) check(bpmf_hip_side_samples_reserve(movies, J.nsims - J.burnin));
    if (ring_u) check(bpmf_hip_side_samples_reserve(users, J.nsims - J.burnin));
    // fold-in: the hyper-parameters every kept iteration of the side ran with, beside the other side's ring
    // (--save-model keeps them for both sides, unless the model is a probit one: fold-in is refused there anyway)
    const bool hyper_u = J.fold_u.n > 0 || (saving && !J.probit), hyper_m = J.fold_m.n > 0 || (saving && !J.probit);
    if (hyper_u) check(bpmf_hip_side_hyper_reserve(users, J.nsims - J.burnin));
    if (hyper_m) check(bpmf_hip_side_hyper_reserve(movies, J.nsims - J.burnin));
    auto set_new = [&](bpmf_hip_side *side, const Job::NewRows &N) {
        if (N.n == 0) return;
        if (N.F.empty()) {
            bool ones = true;
            for (double v : N.Fr.vals) if (v != 1.0) { ones = false; break; }
            static const int32_t none = 0;
            check(bpmf_hip_side_newrows_set_sparse(side, N.n, N.Fr.colptr.data(), N.Fr.rowidx.empty() ? &none : N.Fr.rowidx.data(),
                                                   ones ? nullptr : N.Fr.vals.data(), J.nsims - J.burnin));
        } else
            check(bpmf_hip_side_newrows_set(side, N.n, N.F.data(), J.nsims - J.burnin));
    };
    set_new(users, J.new_u);
    set_new(movies, J.new_m);
    if (J.sharded) {
        check(bpmf_hip_side_set_ranges(movies, J.bm.data()));
        check(bpmf_hip_side_set_ranges(users, J.bu.data()));
    }
    // Sys::add_prop_posterior (c++/sample.cpp:157-174): the K*K x N precisions of this rank's columns
    if (!J.prop_m_lambda.data.empty()) {
        check(bpmf_hip_side_set_prop_posterior(movies, J.prop_m_mu.data.data() + (size_t)K * m0, J.prop_m_lambda.data.data() + (size_t)K * K * m0));
        os << "with propagated posterior" << std::endl;               // c++/sample.cpp:221-222
    }
    print_init(os, "users", J.Mt, J.T.nnz(), J.mean_u);
    if (!J.prop_u_lambda.data.empty()) {
        check(bpmf_hip_side_set_prop_posterior(users, J.prop_u_mu.data.data() + (size_t)K * u0, J.prop_u_lambda.data.data() + (size_t)K * K * u0));
        os << "with propagated posterior" << std::endl;
    }
    // the reference's BPMF_REDUCE build (a compile-time variant there, c++/bpmf.h:30-42; a run-time switch here)
    if (const char *e = getenv("BPMF_REDUCE")) {
        if (atoi(e) != 0) check(bpmf_hip_sys_set_reduce(movies, users, 1));
    }
    const size_t toff = (size_t)J.T.colptr[(size_t)m0];
    {
        const std::vector<int64_t> cp = slice_ptr(J.T, m0, m1);
        check(bpmf_hip_test_create(movies, cp.data(), J.T.rowidx.data() + toff, J.T.vals.data() + toff, &test));
    }
    {   // users.predict(movies) of the reference's loop (c++/bpmf.cpp:190): the users' copy of the test entries (T = Pavg^T of
        // the second Sys, c++/sample.cpp:132-137) is evaluated with every movies.predict(users); nothing prints its results
        const std::vector<int64_t> cp = slice_ptr(J.Tt, u0, u1);
        const size_t off = (size_t)J.Tt.colptr[(size_t)u0];
        check(bpmf_hip_test_create(users, cp.data(), J.Tt.rowidx.data() + off, J.Tt.vals.data() + off, &test_u));
        check(bpmf_hip_test_set_twin(test, test_u));
    }
    double se_u, se_avg_u;
    int64_t num_u = 0;
    auto finish_both = [&](double *se_p, double *se_avg_p, int64_t *num_p) {
        check(bpmf_hip_predict_finish(test, se_p, se_avg_p, num_p));
        check(bpmf_hip_predict_finish(test_u, &se_u, &se_avg_u, &num_u));
    };

    char host[1024];
    gethostname(host, sizeof host);
    os << "hostname: " << host << std::endl;
    os << "pid: " << getpid() << std::endl;
    if (getenv("PBS_JOBID")) os << "jobid: " << getenv("PBS_JOBID") << std::endl;
    os << "num_latent: " << K << std::endl;
    if (J.dtype == BPMF_HIP_F32) os << "arithmetic: fp32 factors / Gram / factorisation (--fp32), fp64 hyper-parameters and sums" << std::endl;
    if (bpmf_hip_kernel_k(K, J.dtype) != K) os << "kernels: num_latent " << bpmf_hip_kernel_k(K, J.dtype) << ", " << bpmf_hip_kernel_k(K, J.dtype) - K << " padded dimensions" << std::endl;
    os << "nprocs: " << J.nranks << std::endl;
    os << "nthrds: " << (J.nthrds > 0 ? J.nthrds : 1) << std::endl;
    os << "nsims: " << J.nsims << std::endl;
    os << "burnin: " << J.burnin << std::endl;
    os << "alpha: " << J.alpha << std::endl;
    if (J.adaptive) {
        os << "noise: adaptive, alpha ~ Gamma(shape " << J.a0 << ", rate " << J.b0 << ") prior, initial alpha " << J.alpha;
        if (J.alpha_max > 0.0) os << ", capped at " << J.alpha_max;
        os << std::endl;
    }
    if (J.probit)
        os << "likelihood: probit, a rating > " << J.probit_threshold << " is a positive label; the RMSE columns compare the latent score "
              "with the raw label and are not an error measure" << std::endl;
    if (J.ordinal) {
        os << "likelihood: ordinal probit, " << J.ord_levels.size() << " levels ";
        for (size_t k = 0; k < J.ord_levels.size(); ++k) os << (k ? "," : "") << J.ord_levels[k];
        os << "; cutpoints ";
        for (size_t k = 0; k < J.ord_cut0.size(); ++k) os << (k ? "," : "") << J.ord_cut0[k];
        os << (J.ord_fixed ? " (fixed)" : " (sampled)") << "; the RMSE columns compare the latent score with the raw value and are not an error measure"
           << std::endl;
    }
    if (J.censored)
        os << "censored: " << J.cens_right << " lower bounds, " << J.cens_left << " upper bounds of " << J.M.nnz() << " training ratings" << std::endl;
    if (J.weighted)
        os << "weights: " << J.w_count << " of " << J.M.nnz() << " training ratings weighted, min " << J.w_min << ", max " << J.w_max << std::endl;
    if (J.robust) os << "robust: Student-t noise, nu = " << J.robust_nu << std::endl;
    if (J.bias) {
        os << "bias: row and column offsets, lambda " << J.bias_lambda;
        if (J.bias_sampled) os << " sampled (" << J.bias_a0 << ", " << J.bias_b0 << ")" << std::endl;
        else os << " fixed" << std::endl;
    }
    if (J.implicit)
        os << "implicit: w0 " << J.implicit_w0 << ", " << J.M.nnz() << " observed of " << nusers << " x " << nmovies << " cells" << std::endl;
    if (linked) {
        os << "side information:";
        if (J.sfeat_u_d > 0) os << " row features sparse D = " << J.sfeat_u_d << " nnz = " << J.sfeat_u.nnz() << ",";
        else if (J.has_feat_u()) os << " row features D = " << J.feat_u.ncols << ",";
        if (J.sfeat_m_d > 0) os << " column features sparse D = " << J.sfeat_m_d << " nnz = " << J.sfeat_m.nnz() << ",";
        else if (J.has_feat_m()) os << " column features D = " << J.feat_m.ncols << ",";
        if (J.sfeat_u_d > 0 || J.sfeat_m_d > 0) os << " CG tol = " << J.link_tol << " max_iter = " << J.link_max_iter << ",";
        os << " lambda_beta = " << J.lambda_beta << "; blocking loop (bpmf_hip_link_sample)" << std::endl;
        if (J.lb_sampled)
            os << "lambda_beta: sampled per side, prior Gamma(shape " << J.lb_a0 << ", rate " << J.lb_b0 << "), initial value " << J.lambda_beta
               << std::endl;
    }
    if (J.new_u.n > 0) os << "new rows: " << J.new_u.n << " (--new-row-features), predicted from their features over the kept samples" << std::endl;
    if (J.new_m.n > 0) os << "new columns: " << J.new_m.n << " (--new-col-features), predicted from their features over the kept samples" << std::endl;
    if (J.fold_u.n > 0) os << "fold-in rows: " << J.fold_u.n << " (--fold-in-rows), " << J.fold_u.Fr.nnz() << " ratings, folded in against the kept samples" << std::endl;
    if (J.fold_m.n > 0) os << "fold-in columns: " << J.fold_m.n << " (--fold-in-cols), " << J.fold_m.Fr.nnz() << " ratings, folded in against the kept samples" << std::endl;
    if (saving) os << "save-model: " << J.save_model << std::endl;
    if (J.diagnose) os << (J.diag_rank ? "diagnose: rank-normalised split-Rhat, bulk and tail ESS of the test predictions" : "diagnose: split-Rhat and ESS of the test predictions") << std::endl;
    if (J.score) os << "score: WAIC of the training cells and log density of the test cells" << std::endl;
    if (!J.iv_levels.empty()) {
        os << "intervals: central predictive intervals of the test cells at";
        for (double l : J.iv_levels) os << " " << level_name(l) << "%";
        os << ", and the calibration of their held-out values" << std::endl;
    }
    if (J.loo) os << "loo: PSIS-LOO cross-validation of the training cells" << std::endl;
    if (J.chain >= 0) os << "chain: " << J.chain << " (random streams of half-iterations " << (long long)J.chain * BPMF_HIP_CHAIN_STRIDE << " ...)" << std::endl;
    os << "update_freq: " << J.update_freq << std::endl;
    if (!J.perm_m.empty()) os << "assignment: greedy (c++/assign.cpp), columns renumbered" << std::endl;
    if (J.sharded) os << "movs domain: [" << m0 << ", " << m1 << ")  users domain: [" << u0 << ", " << u1 << ")" << std::endl;

    const int nsims = J.nsims, burnin = J.burnin;
    double alpha = J.alpha;                                          // (--noise adaptive: redrawn after every iteration)
    const bool probit_eval = J.probit && J.T.nnz() > 0;              // Phi(u . v) of every kept sample, summed on the device (enqueue only)
    long double average_items_sec = 0, average_ratings_sec = 0;
    double rmse = NAN, rmse_avg = NAN, se, se_avg;
    int64_t num_predict = 0;
    int iter = -1;
    const double begin = tick();
    // Sys::print, c++/sample.cpp:101-107
    auto print_line = [&](int it, double rm, double rma, double nu, double nm, double secs) {
        const double items_per_sec = (double)(nusers + nmovies) / secs;
        const double ratings_per_sec = (double)J.M.nnz() / secs;
        char buf[1024];
        int len = snprintf(buf, sizeof buf, "%d: %s iteration %d:\t RMSE: %3.4f\tavg RMSE: %3.4f\tFU(%6.2f)\tFM(%6.2f)\titems/sec: %6.2f\tratings/sec: %6.2fM",
                           rank, (it < burnin) ? "Burnin" : "Sampling", it, rm, rma, std::sqrt(nu), std::sqrt(nm), items_per_sec, ratings_per_sec / 1e6);
        if (J.adaptive && it < (int)J.alpha_trace.size() && len > 0 && len < (int)sizeof buf)
            snprintf(buf + len, sizeof buf - (size_t)len, "\talpha: %.4f\ttrain RMSE: %.4f", J.alpha_trace[(size_t)it], J.train_rmse[(size_t)it]);
        os << buf << "\n" << std::flush;
        average_items_sec += items_per_sec;
        average_ratings_sec += ratings_per_sec;
    };
    // --noise adaptive, after both sides of iteration i: SSE_i on the device, then the alpha of iteration i + 1 on the host.
    // The pipelined loop waits here once per iteration: iteration i + 1 needs this alpha before its first sampler is enqueued.
    auto adapt = [&](int i) {
        double sse = 0.0;
        int64_t n = 0;
        J.alpha_trace.push_back(alpha);
        check(bpmf_hip_train_sse(movies, users, &sse, &n));
        J.train_rmse.push_back(std::sqrt(sse / (double)n));
        if (i + 1 < nsims) check(bpmf_hip_noise_sample(J.a0, J.b0, sse, n, i + (J.chain > 0 ? J.chain * BPMF_HIP_CHAIN_STRIDE : 0), J.alpha_max, &alpha));
    };
    // --ordinal, after both sides of iteration i: the Metropolis-Hastings step of the cutpoints of iteration i + 1 (one pass over the
    // training ratings on the device, the rest on the host; the pipelined loop waits here once per iteration, as adapt does).  The
    // step size follows log s += (accepted - 0.35) / sqrt(iter + 1) during the burn-in unless --ordinal-step gave it.
    const bool ordinal_eval = J.ordinal && J.T.nnz() > 0;
    double ord_s = J.ord_step_given ? J.ord_step : 1.0 / std::sqrt((double)std::max<int64_t>(J.M.nnz(), 1));
    std::vector<double> ord_cut = J.ord_cut0;
    if (J.ordinal && nsims > 0) { J.ord_trace = ord_cut; J.ord_accepted.push_back(0); J.ord_step_trace.push_back(ord_s); }
    auto cut = [&](int i) {
        if (i + 1 >= nsims) return;
        int acc = 0;
        if (!J.ord_fixed) {
            check(bpmf_hip_ordinal_cut_step(movies, users, i + 1, ord_s, &acc));
            if (acc) check(bpmf_hip_side_ordinal_cut_get(movies, ord_cut.data()));
        }
        J.ord_accepted.push_back(acc); J.ord_step_trace.push_back(ord_s);
        J.ord_trace.insert(J.ord_trace.end(), ord_cut.begin(), ord_cut.end());
        if (!J.ord_fixed && !J.ord_step_given && i + 1 < burnin) ord_s = std::exp(std::log(ord_s) + ((acc ? 1.0 : 0.0) - 0.35) / std::sqrt((double)(i + 2)));
    };
    // a model with side information steps both sides through the blocking half-iteration
    // (an implicit model too: bpmf_hip_implicit_sample forms the Gram matrix of the other side first)
    auto sample = [&](bpmf_hip_side *a, bpmf_hip_side *b) {
        check(J.implicit ? bpmf_hip_implicit_sample(a, b, alpha) : linked ? bpmf_hip_link_sample(a, b, alpha) : bpmf_hip_sys_sample(a, b, alpha));
    };
    // (--rank-eval keeps the samples in the rings, which the loop below fills)
    // (--bias: the evaluation of an iteration reads the bias vectors the next one overwrites -- the blocking loop)
    // (--diagnose keeps the samples in the rings too)
    if (J.odirname.empty() && !J.verbose && !linked && !J.implicit && J.rank_eval == 0 && !saving && !J.bias && !J.diagnose && !J.score && J.iv_levels.empty() && !J.loo) {
        // Plain sampling run: the loop of c++/bpmf.cpp:180-198 software-pipelined by one half-iteration.
        // The library only enqueues in bpmf_hip_sys_sample; the line of iteration i-1 (its RMSE sums
        // and norms) is collected after iteration i has been queued, so the device
        // never waits for the host's printing.  The per-iteration rate is the time between two lines.
        double mark = tick(), norm_m = 0.0, norm_u = 0.0;
        for (int i = 0; i < nsims; ++i) {
            check(bpmf_hip_sys_sample(movies, users, alpha));   // movies.sample(users)
            check(bpmf_hip_sys_sample(users, movies, alpha));   // users.sample(movies)
            if (J.adaptive) adapt(i);
            if (probit_eval && i >= burnin) check(bpmf_hip_test_probit_add(test, movies, users));
            if (ordinal_eval && i >= burnin) check(bpmf_hip_test_ordinal_add(test, movies, users));
            if (J.ordinal) cut(i);
            if (i > 0) {
                // norms of iteration i-1 (bpmf_hip_sys_norm waits for THAT half-iteration's sums only: asking bpmf_hip_sys_state
                // here drained each side's pipeline once per iteration -- 83 M against the 100 M samples/s of the same loop
                // without it, bench.py's bpmf_exe record of round 4)
                check(bpmf_hip_sys_norm(movies, i - 1, &norm_m));
                check(bpmf_hip_sys_norm(users, i - 1, &norm_u));
                // the evaluation of iteration i-1 ran beside the two samplers just queued
                finish_both(&se, &se_avg, &num_predict);
                rmse = std::sqrt(se / (double)num_predict);
                rmse_avg = std::sqrt(se_avg / (double)num_predict);
                const double now = tick();
                print_line(i - 1, rmse, rmse_avg, norm_u, norm_m, now - mark);
                mark = now;
            }
            iter = i;
            check(bpmf_hip_predict_launch(test, movies, users, (iter < burnin) ? 0 : (iter - burnin)));
        }
        if (nsims > 0) {
            finish_both(&se, &se_avg, &num_predict);
            rmse = std::sqrt(se / (double)num_predict);
            rmse_avg = std::sqrt(se_avg / (double)num_predict);
            check(bpmf_hip_sys_state(movies, nullptr, &norm_m, nullptr, nullptr, nullptr, nullptr));
            check(bpmf_hip_sys_state(users, nullptr, &norm_u, nullptr, nullptr, nullptr, nullptr));
            print_line(nsims - 1, rmse, rmse_avg, norm_u, norm_m, tick() - mark);
        }
    } else
    for (int i = 0; i < nsims; ++i) {
        static bool cg_warned = false;
        const double start = tick();
        sample(movies, users);                                  // movies.sample(users)
        sample(users, movies);                                  // users.sample(movies)
        if (J.adaptive) adapt(i);
        if (ordinal_eval && i >= burnin) check(bpmf_hip_test_ordinal_add(test, movies, users));
        if (J.ordinal) cut(i);
        iter = i;
        const int n = (iter < burnin) ? 0 : (iter - burnin);
        check(bpmf_hip_predict_launch(test, movies, users, n));
        finish_both(&se, &se_avg, &num_predict);
        rmse = std::sqrt(se / (double)num_predict);
        rmse_avg = std::sqrt(se_avg / (double)num_predict);
        const double stop = tick();
        double norm_u, norm_m;
        check(bpmf_hip_sys_state(users, nullptr, &norm_u, nullptr, nullptr, nullptr, nullptr));
        check(bpmf_hip_sys_state(movies, nullptr, &norm_m, nullptr, nullptr, nullptr, nullptr));
        print_line(iter, rmse, rmse_avg, norm_u, norm_m, stop - start);
        if (J.diagnose && iter >= burnin) { J.dg_trace[0].push_back(rmse); J.dg_trace[1].push_back(std::sqrt(norm_u)); J.dg_trace[2].push_back(std::sqrt(norm_m)); }

        // aggrMu / aggrLambda of this rank's columns, on the device (c++/sample.cpp:364-368)
        if (aggregate && iter >= burnin) { check(bpmf_hip_side_aggr_add(users)); check(bpmf_hip_side_aggr_add(movies)); }
        if (J.robust && aggregate && iter >= burnin) check(bpmf_hip_side_robust_add(movies));
        if (J.bias && aggregate && iter >= burnin) { check(bpmf_hip_side_bias_add(users)); check(bpmf_hip_side_bias_add(movies)); }
        if (ring_u && iter >= burnin) check(bpmf_hip_side_samples_add(users));
        if (ring_m && iter >= burnin) check(bpmf_hip_side_samples_add(movies));
        if (hyper_u && iter >= burnin) check(bpmf_hip_side_hyper_add(users, J.adaptive ? J.alpha_trace[(size_t)i] : alpha, nullptr, nullptr));
        if (hyper_m && iter >= burnin) check(bpmf_hip_side_hyper_add(movies, J.adaptive ? J.alpha_trace[(size_t)i] : alpha, nullptr, nullptr));
        if (J.new_u.n > 0 && iter >= burnin) check(bpmf_hip_side_newrows_add(users, movies));
        if (J.new_m.n > 0 && iter >= burnin) check(bpmf_hip_side_newrows_add(movies, users));
        if (probit_eval && iter >= burnin) check(bpmf_hip_test_probit_add(test, movies, users));
        if (!cg_warned && (J.sfeat_u_d > 0 || J.sfeat_m_d > 0)) {       // CG at max_iter with a column still active: said once
            int hit_u = 0, hit_m = 0;
            if (J.sfeat_u_d > 0) check(bpmf_hip_side_link_cg_stats(users, nullptr, nullptr, nullptr, &hit_u));
            if (J.sfeat_m_d > 0) check(bpmf_hip_side_link_cg_stats(movies, nullptr, nullptr, nullptr, &hit_m));
            if (hit_u || hit_m) {
                std::cerr << "warning: the CG draw of the link matrix reached --link-max-iter " << J.link_max_iter << " in iteration " << iter
                          << " before its residual fell below --link-tol " << J.link_tol << std::endl;
                cg_warned = true;
            }
        }
        if (J.lb_sampled) {
            double lam = 0.0;
            if (J.has_feat_u()) { check(bpmf_hip_side_link_lambda_get(users, &lam, nullptr, nullptr)); J.lb_trace_u.push_back(lam); }
            if (J.has_feat_m()) { check(bpmf_hip_side_link_lambda_get(movies, &lam, nullptr, nullptr)); J.lb_trace_m.push_back(lam); }
        }
        if (linked && iter >= burnin) {
            if (J.has_feat_u()) check(bpmf_hip_side_link_add(users));
            if (J.has_feat_m()) check(bpmf_hip_side_link_add(movies));
        }
        // (-v: the replicas of both factor matrices are complete on every rank -- the all-gather form of the exchange;
        // users.bcast() / movies.bcast() of c++/bpmf.cpp:202-203 have nothing left to do)
        if (J.verbose && rank == 0) {
            Dense d;
            d.nrows = K;
            d.ncols = nusers; d.data.resize((size_t)K * nusers);
            check(bpmf_hip_side_get_items(users, d.data.data()));
            if (!J.perm_u.empty()) permute_columns(d.data, K, inverse(J.perm_u));
            bpmf::io::write_dense(J.odirname + "/U-" + std::to_string(i) + ".ddm", d);
            d.ncols = nmovies; d.data.resize((size_t)K * nmovies);
            check(bpmf_hip_side_get_items(movies, d.data.data()));
            if (!J.perm_m.empty()) permute_columns(d.data, K, inverse(J.perm_m));
            bpmf::io::write_dense(J.odirname + "/V-" + std::to_string(i) + ".ddm", d);
        }
    }
    const double elapsed = tick() - begin;

    // movies.predict(users, true) once more with the same iter (c++/bpmf.cpp:225,242: SURVEY Q6)
    if (nsims > 0) {
        const int n = (iter < burnin) ? 0 : (iter - burnin);
        check(bpmf_hip_predict_launch(test, movies, users, n));
        finish_both(&se, &se_avg, &num_predict);
        rmse_avg = std::sqrt(se_avg / (double)num_predict);
    }
    if (!J.odirname.empty()) {                                        // this rank's slice of Pavg / Pm2 and of the posterior
        const size_t tn = (size_t)(J.T.colptr[(size_t)m1] - J.T.colptr[(size_t)m0]);
        if (tn) check(bpmf_hip_test_get(test, J.pavg.data() + toff, J.pm2.data() + toff));
        const int nsamples = nsims - burnin;
        if (nsamples > 0) {                                           // Sys::finalize_mu_lambda (c++/bpmf.cpp:281-295), batched on the device
            check(bpmf_hip_side_aggr_finalize(users, nsamples, J.u_mu.data() + (size_t)K * u0, J.u_lambda.data() + (size_t)K * K * u0));
            check(bpmf_hip_side_aggr_finalize(movies, nsamples, J.m_mu.data() + (size_t)K * m0, J.m_lambda.data() + (size_t)K * K * m0));
        }
    }
    if (J.bias && aggregate && nsims > 0) {
        double cur = 0.0;
        J.bias_lam_u.resize((size_t)nsims); J.bias_lam_m.resize((size_t)nsims);
        check(bpmf_hip_side_bias_lambda_get(users, &cur, J.bias_lam_u.data(), nsims, nullptr, nullptr));
        check(bpmf_hip_side_bias_lambda_get(movies, &cur, J.bias_lam_m.data(), nsims, nullptr, nullptr));
    }
    if (J.bias && aggregate && nsims > burnin) {                     // one rank (main refuses -g)
        J.bias_u.resize((size_t)std::max<int64_t>(nusers, 1)); J.bias_m.resize((size_t)std::max<int64_t>(nmovies, 1));
        check(bpmf_hip_side_bias_mean(users, J.bias_u.data(), nullptr));
        check(bpmf_hip_side_bias_mean(movies, J.bias_m.data(), nullptr));
        J.bias_u.resize((size_t)nusers); J.bias_m.resize((size_t)nmovies);
    }
    if (J.robust && aggregate && nsims > burnin) {                   // one rank (main refuses -g)
        J.robust_w.resize((size_t)std::max<int64_t>(J.M.nnz(), 1));
        check(bpmf_hip_side_robust_get(movies, J.robust_w.data(), nullptr, nullptr));
        J.robust_w.resize((size_t)J.M.nnz());
    }
    if (linked && nsims > burnin) {                                  // one rank (main refuses -g)
        if (J.has_feat_u()) { J.beta_u.resize((size_t)(J.sfeat_u_d > 0 ? J.sfeat_u_d : J.feat_u.ncols) * K); check(bpmf_hip_side_link_mean(users, J.beta_u.data(), nullptr)); }
        if (J.has_feat_m()) { J.beta_m.resize((size_t)(J.sfeat_m_d > 0 ? J.sfeat_m_d : J.feat_m.ncols) * K); check(bpmf_hip_side_link_mean(movies, J.beta_m.data(), nullptr)); }
    }
    if (probit_eval && nsims > burnin) {                             // one rank (main refuses -g)
        J.prob.resize((size_t)J.T.nnz());
        check(bpmf_hip_test_probit_get(test, J.prob.data(), nullptr));
        std::vector<double> label(J.prob.size());
        double sq = 0.0;
        for (size_t q = 0; q < label.size(); ++q) {
            label[q] = J.T.vals[q] > J.probit_threshold ? 1.0 : 0.0;
            sq += (J.prob[q] - label[q]) * (J.prob[q] - label[q]);
        }
        check(bpmf_hip_auc(J.prob.data(), label.data(), (int64_t)label.size(), 0.5, &J.auc));
        J.brier = sq / (double)label.size();
    }
    if (ordinal_eval && nsims > burnin) {                            // one rank (main refuses -g)
        const size_t C = J.ord_levels.size(), n = (size_t)J.T.nnz();
        J.cat_prob.resize(n * C);
        check(bpmf_hip_test_ordinal_get(test, J.cat_prob.data(), nullptr, nullptr));
        double sq = 0.0, lp = 0.0;
        size_t hit = 0;
        for (size_t q = 0; q < n; ++q) {
            const double *p = &J.cat_prob[q * C];
            double e = 0.0;
            size_t best = 0, truth = 0;
            for (size_t k = 0; k < C; ++k) {
                e += J.ord_levels[k] * p[k];
                if (p[k] > p[best]) best = k;
                if (J.ord_levels[k] == J.T.vals[q]) truth = k;
            }
            sq += (e - J.T.vals[q]) * (e - J.T.vals[q]);
            hit += best == truth;
            lp += std::log(p[truth]);
        }
        J.ord_rmse = std::sqrt(sq / (double)n); J.ord_accuracy = (double)hit / (double)n; J.ord_logp = lp / (double)n;
    }
    serve_rank(J, users, movies);                                    // --topn, --rank-eval: one rank (main refuses -g > 1)
    serve_similar(J, users, movies);
    serve_diag(J, users, movies, J.T);
    if (J.diagnose) {                                                // the scalar traces through the same estimator
        const size_t S = J.dg_trace[0].size();
        std::vector<double> tr, rh(3);
        for (const std::vector<double> &t : J.dg_trace) tr.insert(tr.end(), t.begin(), t.end());
        check(bpmf_hip_diag_traces(ctx, 3, (int)S, tr.data(), rh.data(), J.dg_trace_ess));
    }
    if (J.score || !J.iv_levels.empty() || J.loo) {                  // the alpha every kept iteration ran with
        J.sc_alpha.clear();
        if (J.adaptive) for (int it = burnin; it < nsims; ++it) J.sc_alpha.push_back(J.alpha_trace[(size_t)it]);
        else J.sc_alpha.push_back(J.probit ? 1.0 : J.alpha);
        serve_score(J, users, movies, J.T.nnz() > 0 ? &J.T : nullptr, &J.M);     // (no test cell: no test line)
        serve_intervals(J, users, movies, J.T);
        serve_loo(J, users, movies, J.M);
    }
    // the new entities against every column of the other side, in query ranges: the device holds one range's block at a time
    auto predict_new = [&](bpmf_hip_side *side, bpmf_hip_side *cand, Job::NewRows &N, int64_t nc, bool by_new) {
        if (N.n == 0) return;
        const double t0 = tick();
        if (N.dense_out) {
            N.mean.resize((size_t)N.n * (size_t)nc); N.std.resize(N.mean.size());
            const int64_t step = std::max<int64_t>(64, ((int64_t)1 << 24) / std::max<int64_t>(nc, 1) / 64 * 64);
            for (int64_t q0 = 0; q0 < N.n; q0 += step) {
                const int64_t q1 = std::min(N.n, q0 + step);
                check(bpmf_hip_newrows_predict(side, cand, J.mean_m, q0, q1, 0, nc, N.mean.data() + (size_t)q0 * nc, N.std.data() + (size_t)q0 * nc));
            }
        }
        if (J.topn > 0) {
            N.new_are_queries = by_new;
            const int64_t nq = by_new ? N.n : nc;
            N.topn_idx.resize((size_t)nq * J.topn); N.topn_mean.resize(N.topn_idx.size()); N.topn_std.resize(N.topn_idx.size());
            check(bpmf_hip_newrows_topn(side, cand, J.mean_m, J.topn, by_new ? 1 : 0, N.topn_idx.data(), N.topn_mean.data(), N.topn_std.data()));
        }
        std::cerr << "new " << (side == users ? "rows" : "columns") << ": " << N.n << " x " << nc << " predictions, " << (tick() - t0) * 1e3 << " ms" << std::endl;
    };
    predict_new(users, movies, J.new_u, nmovies, !J.topn_by_cols);   // --topn-by rows: the new rows are the queries
    predict_new(movies, users, J.new_m, nusers, J.topn_by_cols);     // --topn-by cols: the new columns are the queries
    serve_fold(J, users, movies);
    if (saving) {                                                    // one rank (main refuses -g); the ORIGINAL numbering, as the -o writers
        const double t0 = tick();
        bpmf::io::Model m;
        m.K = K; m.S = nsims - burnin; m.rows = nusers; m.cols = nmovies; m.mean_rating = J.mean_m; m.alpha = J.alpha;
        m.probit = J.probit; m.probit_threshold = J.probit ? J.probit_threshold : 0.0; m.f32 = J.dtype == BPMF_HIP_F32; m.hyper = hyper_u && hyper_m;
        const size_t sk = (size_t)m.S * (size_t)K, h = 1 + (size_t)K + (size_t)K * K;
        m.U.resize(sk * (size_t)nusers); m.V.resize(sk * (size_t)nmovies);
        check(bpmf_hip_side_samples_get(users, 0, m.S, m.U.data()));
        check(bpmf_hip_side_samples_get(movies, 0, m.S, m.V.data()));
        if (!J.perm_u.empty()) { permute_columns(m.U, (int64_t)sk, inverse(J.perm_u)); permute_columns(m.V, (int64_t)sk, inverse(J.perm_m)); }
        auto hyper = [&](bpmf_hip_side *side, std::vector<double> &out) {      // column s = alpha_s, mu_s, Lambda_s
            std::vector<double> a((size_t)m.S), mu((size_t)m.S * K), lam((size_t)m.S * K * K);
            check(bpmf_hip_side_hyper_get(side, a.data(), mu.data(), lam.data()));
            out.resize(h * (size_t)m.S);
            for (size_t sm = 0; sm < (size_t)m.S; ++sm) {
                out[sm * h] = a[sm];
                memcpy(&out[sm * h + 1], &mu[sm * K], sizeof(double) * (size_t)K);
                memcpy(&out[sm * h + 1 + K], &lam[sm * K * K], sizeof(double) * (size_t)K * K);
            }
        };
        if (m.hyper) { hyper(users, m.Uh); hyper(movies, m.Vh); }
        try { bpmf::io::write_model(J.save_model, m); } catch (const std::exception &e) { die(e.what()); }
        std::cerr << "save-model: " << m.S << " samples of " << nusers << " + " << nmovies << " columns, " << (tick() - t0) * 1e3 << " ms" << std::endl;
    }
    if (rank == 0) {
        J.elapsed = elapsed; J.rmse_avg = rmse_avg; J.num_predict = num_predict;
        J.average_items_sec = average_items_sec; J.average_ratings_sec = average_ratings_sec;
    }
    bpmf_hip_test_destroy(test);
    bpmf_hip_test_destroy(test_u);
    bpmf_hip_side_destroy(movies);
    bpmf_hip_side_destroy(users);
    bpmf_hip_ctx_destroy(ctx);
}

}  // namespace

// --tensor: the Gibbs loop of the tensor model (bpmf_amd.tensor_gibbs is the same loop): per iteration every mode, last mode first --
// the hyper-parameters of the mode at counter `it` from its cov, bpmf_hip_tensor_sample, cov from the sums -- then the test entries.
static int run_tensor(const std::string &file, const std::string &test_file, const std::string &dims_text, bool dims_given, int K, int nsims, int burnin,
               double alpha, const std::string &odir)
{
    using bpmf::io::Tns;
    Tns A, T;
    try {
        A = bpmf::io::read_tns(file);
        if (!test_file.empty()) T = bpmf::io::read_tns(test_file);
    } catch (const std::exception &e) { die(e.what()); }
    int64_t dims[3];
    for (int m = 0; m < 3; ++m) dims[m] = std::max(A.dims[m], T.dims[m]);
    if (dims_given) {
        long long d[3] = {0, 0, 0};
        char tail = 0;
        if (sscanf(dims_text.c_str(), "%lld,%lld,%lld%c", &d[0], &d[1], &d[2], &tail) != 3 || d[0] < 1 || d[1] < 1 || d[2] < 1)
            die("--tensor-dims expects I,J,T, three sizes >= 1, not '" + dims_text + "'");
        for (int m = 0; m < 3; ++m) {
            if (d[m] < dims[m])
                die("--tensor-dims " + dims_text + ": mode " + std::to_string(m + 1) + " has size " + std::to_string(d[m]) + ", the files hold the index " + std::to_string(dims[m]));
            dims[m] = d[m];
        }
    }
    const int64_t nnz = (int64_t)A.vals.size(), nnzt = (int64_t)T.vals.size();
    if (nnz == 0) die("the training tensor is empty");
    double mean = 0.0;
    for (double v : A.vals) mean += v;
    mean /= (double)nnz;
    std::ostream &os = std::cout;
    os << "tensor: " << dims[0] << " x " << dims[1] << " x " << dims[2] << ", " << nnz << " ratings, " << nnzt << " test" << std::endl;
    os << "num_latent: " << K << "\n" << "mean rating: " << mean << "\n" << "alpha: " << alpha << std::endl;

    bpmf_hip_ctx *ctx = nullptr;
    bpmf_hip_tensor *tensor = nullptr;
    bpmf_hip_tensor_test *tt = nullptr;
    check(bpmf_hip_ctx_create(0, K, nullptr, &ctx));
    check(bpmf_hip_tensor_create(ctx, 3, dims, nnz, A.idx[0].data(), A.idx[1].data(), A.idx[2].data(), A.vals.data(), mean, &tensor));
    if (nnzt > 0) check(bpmf_hip_tensor_test_create(tensor, nnzt, T.idx[0].data(), T.idx[1].data(), T.idx[2].data(), T.vals.data(), &tt));
    const size_t kk = (size_t)K * K;
    std::vector<double> cov[3], mu((size_t)K), LU(kk), LF(kk), sum((size_t)K), prod(kk);
    for (auto &c : cov) c.assign(kk, 0.0);
    double rmse = 0.0, rmse_avg = 0.0, items_sec_sum = 0.0;
    int kept = 0;
    for (int it = 0; it < nsims; ++it) {
        const double t0 = tick();
        double norm[3] = {0, 0, 0};
        for (int m = 2; m >= 0; --m) {
            if (bpmf_hyper_sample(K, dims[m], cov[m].data(), nullptr, (uint32_t)it, mu.data(), LU.data(), LF.data())) die("the hyper-parameter draw failed");
            check(bpmf_hip_tensor_sample(tensor, m, it, alpha, mu.data(), LF.data(), sum.data(), prod.data(), &norm[m]));
            bpmf_cov_from_sums(K, dims[m], sum.data(), prod.data(), cov[m].data());
        }
        if (tt) {
            double se = 0.0, se_avg = 0.0;
            int64_t count = 0;
            check(bpmf_hip_tensor_predict(tt, it < burnin ? 0 : it - burnin, &se, &se_avg, &count));
            rmse = std::sqrt(se / (double)count); rmse_avg = std::sqrt(se_avg / (double)count);
        }
        if (it >= burnin && !odir.empty()) {
            for (int m = 0; m < 3; ++m) check(bpmf_hip_side_aggr_add(bpmf_hip_tensor_side(tensor, m)));
            ++kept;
        }
        const double items_per_sec = (double)(dims[0] + dims[1] + dims[2]) / (tick() - t0);
        items_sec_sum += items_per_sec;
        char buf[512];
        snprintf(buf, sizeof buf, "0: %s iteration %d:\t RMSE: %3.4f\tavg RMSE: %3.4f\tF1(%6.2f)\tF2(%6.2f)\tF3(%6.2f)\titems/sec: %6.2f",
                 (it < burnin) ? "Burnin" : "Sampling", it, rmse, rmse_avg, std::sqrt(norm[0]), std::sqrt(norm[1]), std::sqrt(norm[2]), items_per_sec);
        os << buf << "\n" << std::flush;
    }
    if (!odir.empty()) {
        try {
            for (int m = 0; m < 3 && kept > 0; ++m) {
                Dense d;
                d.nrows = K; d.ncols = dims[m]; d.data.resize((size_t)K * (size_t)dims[m]);
                std::vector<double> lambda(kk * (size_t)dims[m]);
                check(bpmf_hip_side_aggr_finalize(bpmf_hip_tensor_side(tensor, m), kept, d.data.data(), lambda.data()));
                bpmf::io::write_dense(odir + "/mode" + std::to_string(m + 1) + "-mu.ddm", d);
            }
            if (tt) {
                Tns P = T;
                std::vector<double> pm2((size_t)nnzt);
                check(bpmf_hip_tensor_test_get(tt, P.vals.data(), pm2.data()));
                bpmf::io::write_tns(odir + "/Pavg.tns", P);
                P.vals = pm2;
                bpmf::io::write_tns(odir + "/Pm2.tns", P);
            }
        } catch (const std::exception &e) { die(e.what()); }
    }
    os << "Final Avg RMSE: " << rmse_avg << std::endl;
    os << "Average items/sec: " << items_sec_sum / std::max(nsims, 1) << std::endl;
    check(bpmf_hip_tensor_test_destroy(tt));
    check(bpmf_hip_tensor_destroy(tensor));
    check(bpmf_hip_ctx_destroy(ctx));
    return 0;
}

// --model DIR: serves a saved model (bpmf --save-model, bpmf_amd.save_model) without a chain.  The model is read
// and everything that can be refused is refused before a GPU is touched; then a fp64 context with the model's num_latent, both sides
// from the training matrix (-n: the cells the rankings exclude) or from empty matrices, the sample rings and the hyper rings loaded,
// and what was asked for -- --predict, --topn, --rank-eval, --fold-in-rows / -cols -- through the code a training run serves them with.
static int run_model(Job &J, const std::string &dir, const std::string &fname, const std::string &probename, const std::string &predict_file,
                     bool thr_given, double thr, const std::string &fold_in_rows, const std::string &fold_in_cols, bool d_given, int d)
{
    // DIR may be a list D0,D1,.. of chains of one model: pooled along the sample axis in list order (bpmf_amd.pool_models)
    bpmf::io::Model m;
    int chains = 0;
    for (size_t from = 0; from <= dir.size();) {
        const size_t to = std::min(dir.find(',', from), dir.size());
        const std::string one = dir.substr(from, to - from);
        from = to + 1;
        if (one.empty()) die("--model: an empty directory name in the list '" + dir + "'");
        bpmf::io::Model c;
        try { c = bpmf::io::read_model(one); } catch (const std::exception &e) { die(e.what()); }
        if (chains++ == 0) { m = std::move(c); continue; }
        const int S0 = m.S / (chains - 1);                           // samples of one chain
        const char *what = c.rows != m.rows || c.cols != m.cols ? "shape" : c.K != m.K ? "num_latent" : c.probit != m.probit || c.probit_threshold != m.probit_threshold ? "likelihood" :
                           c.mean_rating != m.mean_rating ? "mean rating" : c.f32 != m.f32 ? "dtype" : c.S != S0 ? "samples" : c.hyper != m.hyper ? "the presence of the hyper files" : nullptr;
        if (what) die("--model: " + one + " differs from " + dir.substr(0, dir.find(',')) + " in " + what + " (chains of one model are pooled)");
        const size_t sk = (size_t)S0 * (size_t)m.K;                  // doubles of one chain per row / column
        for (int prev = 0; prev < chains - 1; ++prev) {
            bool same = true;
            for (int64_t r = 0; r < m.rows && same; ++r)
                same = memcmp(&m.U[(size_t)r * (size_t)m.S * (size_t)m.K + (size_t)prev * sk], &c.U[(size_t)r * sk], sizeof(double) * (size_t)m.K) == 0;
            if (same) die("--model: " + one + " has the first kept sample of chain " + std::to_string(prev) + " of the list, byte for byte: the same chain twice (bpmf --chain c makes them differ)");
        }
        auto append = [&](std::vector<double> &all, const std::vector<double> &add, int64_t n) {   // n blocks: (all's block, add's block) interleaved
            const size_t a = all.size() / (size_t)n, b = add.size() / (size_t)n;
            std::vector<double> out; out.reserve(all.size() + add.size());
            for (int64_t i = 0; i < n; ++i) {
                out.insert(out.end(), all.begin() + (ptrdiff_t)((size_t)i * a), all.begin() + (ptrdiff_t)((size_t)(i + 1) * a));
                out.insert(out.end(), add.begin() + (ptrdiff_t)((size_t)i * b), add.begin() + (ptrdiff_t)((size_t)(i + 1) * b));
            }
            all.swap(out);
        };
        append(m.U, c.U, m.rows); append(m.V, c.V, m.cols);
        if (m.hyper) { m.Uh.insert(m.Uh.end(), c.Uh.begin(), c.Uh.end()); m.Vh.insert(m.Vh.end(), c.Vh.begin(), c.Vh.end()); }
        m.S += c.S;
    }
    J.dg_chains = chains;
    if (chains > 1) J.diag_rank = J.diagnose;                        // --diagnose under a pooled model is the multi-chain estimator
    const int K = m.K;
    if (d_given && d != K) die("-d " + std::to_string(d) + " differs from the num_latent " + std::to_string(K) + " of the model " + dir);
    if (J.score && m.S < 2) die("--score needs at least 2 samples, the model " + dir + " holds " + std::to_string(m.S));
    if (J.score && !m.probit && !(m.alpha > 0.0) && !m.hyper) die("--score needs a model with alpha > 0 (the noise precision of its likelihood)");
    if (J.loo && (m.S < 2 || m.S > BPMF_HIP_LOO_MAX_SAMPLES))
        die("--loo needs 2 .. " + std::to_string(BPMF_HIP_LOO_MAX_SAMPLES) + " samples, the model " + dir + " holds " + std::to_string(m.S));
    if (J.loo && !m.probit && !(m.alpha > 0.0) && !m.hyper) die("--loo needs a model with alpha > 0 (the noise precision of its likelihood)");
    if (!J.iv_levels.empty() && m.probit) die("--intervals: " + dir + " is a probit model (its predictive is a probability, not an interval)");
    if (!J.iv_levels.empty() && m.S > BPMF_HIP_INTERVAL_MAX_SAMPLES)
        die("--intervals takes at most " + std::to_string(BPMF_HIP_INTERVAL_MAX_SAMPLES) + " samples, the model " + dir + " holds " + std::to_string(m.S));
    if (!J.iv_levels.empty() && !(m.alpha > 0.0) && !m.hyper) die("--intervals needs a model with alpha > 0 (the noise precision of its likelihood)");
    if (J.diagnose && (m.S / chains < 8 || m.S > BPMF_HIP_DIAG_MAX_SAMPLES))
        die(chains > 1 ? "--diagnose needs 8 or more samples per chain and " + std::to_string(BPMF_HIP_DIAG_MAX_SAMPLES) + " at most in all, the models " + dir + " hold " +
                         std::to_string(chains) + " x " + std::to_string(m.S / chains)
                       : "--diagnose needs 8 .. " + std::to_string(BPMF_HIP_DIAG_MAX_SAMPLES) + " samples, the model " + dir + " holds " + std::to_string(m.S));
    for (const std::string *f : {&fold_in_rows, &fold_in_cols}) {
        if (f->empty()) continue;
        const std::string w = f == &fold_in_rows ? "--fold-in-rows" : "--fold-in-cols";
        if (m.probit) die(w + ": " + dir + " is a probit model, which is saved without hyper files: labels would need a latent iteration of their own");
        if (!m.hyper) die(w + ": " + dir + " was saved without hyper files (model.txt: hyper 0)");
    }
    if (J.topn_kind == BPMF_HIP_SCORE_PROB || J.topn_kind == BPMF_HIP_SCORE_EI) {
        if (!m.probit && !(m.alpha > 0.0)) die("--topn-score needs a model with alpha > 0 (sigma = 1 / sqrt(alpha))");
        J.topn_sigma = m.probit ? 1.0 : 1.0 / std::sqrt(m.alpha);
    }
    const int64_t nusers = m.rows, nmovies = m.cols;
    try {
        if (!fname.empty()) J.M = bpmf::io::read_sparse(fname);
        if (!probename.empty()) J.T = bpmf::io::read_sparse(probename);
    } catch (const std::exception &e) { die(e.what()); }
    if (!fname.empty()) {                                            // the shape a training run gives both: the larger of the two files
        const int64_t r = std::max(J.M.nrows, J.T.nrows), c = std::max(J.M.ncols, J.T.ncols);
        if (r != nusers || c != nmovies)
            die("-n " + fname + (probename.empty() ? "" : " with -p " + probename) + " is " + std::to_string(r) + " x " + std::to_string(c) + ", the model " + dir +
                " is " + std::to_string(nusers) + " x " + std::to_string(nmovies));
    } else {
        J.M.colptr.assign((size_t)nmovies + 1, 0);
    }
    bpmf::io::resize(J.M, nusers, nmovies);
    if (!probename.empty()) {
        if (J.T.nrows > nusers || J.T.ncols > nmovies) die("-p " + probename + " is larger than the model " + dir);
        bpmf::io::resize(J.T, nusers, nmovies);
    } else {
        J.T.colptr.assign((size_t)nmovies + 1, 0); J.T.nrows = nusers; J.T.ncols = nmovies;
    }
    J.Mt = bpmf::io::transpose(J.M);
    J.Tt = bpmf::io::transpose(J.T);
    J.K = K; J.dtype = BPMF_HIP_F64; J.mean_m = J.mean_u = m.mean_rating; J.alpha = m.alpha; J.probit = m.probit;
    build_rank_lists(J);
    read_fold(J, fold_in_rows, true, J.fold_u);
    read_fold(J, fold_in_cols, false, J.fold_m);
    Csc P;                                                           // --predict FILE: the cells, in the reader's order
    if (!predict_file.empty()) {
        try { P = bpmf::io::read_sparse(predict_file); } catch (const std::exception &e) { die(e.what()); }
        if (P.nrows > nusers || P.ncols > nmovies)
            die("--predict: " + predict_file + " is " + std::to_string(P.nrows) + " x " + std::to_string(P.ncols) + ", the model " + dir + " is " +
                std::to_string(nusers) + " x " + std::to_string(nmovies));
    }
    const bool want_prob = m.probit || thr_given;
    const double pt = thr_given ? thr : 0.0, psigma = m.probit ? 1.0 : (m.alpha > 0.0 ? 1.0 / std::sqrt(m.alpha) : 0.0);
    if (!predict_file.empty() && thr_given && !m.probit && !(m.alpha > 0.0)) die("--predict-threshold needs a model with alpha > 0 (sigma = 1 / sqrt(alpha))");

    std::cout << "model: " << dir << ", " << nusers << " x " << nmovies << ", num_latent " << K << ", " << m.S << " samples, " << (m.probit ? "probit" : "gaussian")
              << (chains > 1 ? ", " + std::to_string(chains) + " chains" : std::string()) << std::endl;
    int device = 0;
    if (const char *e = getenv("BPMF_HIP_DEVICES")) device = atoi(e);
    bpmf_hip_ctx *ctx = nullptr;
    bpmf_hip_side *movies = nullptr, *users = nullptr;
    const double t0 = tick();
    static const int32_t none = 0; static const double zero = 0.0;
    check(bpmf_hip_ctx_create_ex(device, K, BPMF_HIP_F64, nullptr, &ctx));
    check(bpmf_hip_side_create(ctx, nmovies, nusers, 0, nmovies, J.M.colptr.data(), J.M.rowidx.empty() ? &none : J.M.rowidx.data(),
                               J.M.vals.empty() ? &zero : J.M.vals.data(), J.mean_m, &movies));
    check(bpmf_hip_side_create(ctx, nusers, nmovies, 0, nusers, J.Mt.colptr.data(), J.Mt.rowidx.empty() ? &none : J.Mt.rowidx.data(),
                               J.Mt.vals.empty() ? &zero : J.Mt.vals.data(), J.mean_u, &users));
    check(bpmf_hip_side_samples_reserve(users, m.S)); check(bpmf_hip_side_samples_set(users, m.S, m.U.data()));
    check(bpmf_hip_side_samples_reserve(movies, m.S)); check(bpmf_hip_side_samples_set(movies, m.S, m.V.data()));
    if (m.hyper && !m.probit) {
        const size_t h = 1 + (size_t)K + (size_t)K * K;
        for (int which = 0; which < 2; ++which) {
            bpmf_hip_side *side = which ? movies : users;
            const std::vector<double> &H = which ? m.Vh : m.Uh;
            check(bpmf_hip_side_hyper_reserve(side, m.S));
            for (size_t sm = 0; sm < (size_t)m.S; ++sm) check(bpmf_hip_side_hyper_add(side, H[sm * h], &H[sm * h + 1], &H[sm * h + 1 + K]));
        }
    }
    std::cerr << "model: loaded in " << (tick() - t0) * 1e3 << " ms" << std::endl;

    if (!predict_file.empty()) {
        const double t1 = tick();
        const size_t n = (size_t)P.nnz();
        std::vector<int32_t> q(std::max<size_t>(n, 1)), c(std::max<size_t>(n, 1));
        for (int64_t col = 0; col < P.ncols; ++col)
            for (int64_t at = P.colptr[(size_t)col]; at < P.colptr[(size_t)col + 1]; ++at) { q[(size_t)at] = P.rowidx[(size_t)at]; c[(size_t)at] = (int32_t)col; }
        std::vector<double> mean(std::max<size_t>(n, 1)), sd(std::max<size_t>(n, 1)), prob(std::max<size_t>(n, 1));
        check(bpmf_hip_predict_cells(users, movies, J.mean_m, (int64_t)n, q.data(), c.data(), want_prob ? 1 : 0, pt, psigma, mean.data(), sd.data(), prob.data()));
        const std::string name = J.odirname + "/predict.csv";
        FILE *f = fopen(name.c_str(), "w");
        if (!f) die("cannot write " + name);
        fprintf(f, want_prob ? "row,col,mean,std,prob\n" : "row,col,mean,std\n");
        for (size_t i = 0; i < n; ++i) {
            if (want_prob) fprintf(f, "%lld,%lld,%.17g,%.17g,%.17g\n", (long long)q[i] + 1, (long long)c[i] + 1, mean[i], sd[i], prob[i]);
            else fprintf(f, "%lld,%lld,%.17g,%.17g\n", (long long)q[i] + 1, (long long)c[i] + 1, mean[i], sd[i]);
        }
        if (fclose(f) != 0) die("cannot write " + name);
        std::cerr << "predict: " << n << " cells, " << (tick() - t1) * 1e3 << " ms" << std::endl;
    }
    serve_rank(J, users, movies);
    serve_similar(J, users, movies);
    serve_diag(J, users, movies, P);                                 // --predict FILE --diagnose: FILE's cells
    if (J.score || !J.iv_levels.empty() || J.loo) {                  // --predict FILE --score / --intervals: FILE's values are the observations; -n TRAIN: its WAIC
        J.probit_threshold = m.probit_threshold;
        J.sc_alpha.clear();
        if (m.hyper && !m.probit) for (size_t sm = 0; sm < (size_t)m.S; ++sm) J.sc_alpha.push_back(m.Uh[sm * (1 + (size_t)K + (size_t)K * K)]);
        else J.sc_alpha.push_back(m.probit ? 1.0 : m.alpha);
        serve_score(J, users, movies, predict_file.empty() ? nullptr : &P, fname.empty() ? nullptr : &J.M);
        serve_intervals(J, users, movies, P);
        serve_loo(J, users, movies, J.M);
    }
    serve_fold(J, users, movies);
    bpmf_hip_side_destroy(movies);
    bpmf_hip_side_destroy(users);
    bpmf_hip_ctx_destroy(ctx);

    write_topn(J);
    write_similar(J);
    write_diag(J);
    print_diag(std::cout, J, false);
    write_score(J, &P, &J.M);
    print_score(std::cout, J);
    write_intervals(J);
    print_intervals(std::cout, J);
    write_loo(J, J.M);
    print_loo(std::cout, J);
    const RankMetrics rkm = write_ranks(J);
    write_new(J, J.fold_u, true, nmovies, "foldin");
    write_new(J, J.fold_m, false, nusers, "foldin");
    if (J.rank_eval > 0) {
        std::cout << "Final recall@" << J.rank_eval << ": " << rkm.recall << std::endl;
        std::cout << "Final NDCG@" << J.rank_eval << ": " << rkm.ndcg << std::endl;
        std::cout << "Final MRR: " << rkm.mrr << std::endl;
        std::cout << "Final MPR: " << rkm.mpr << std::endl;
        std::cout << "Final rank AUC: " << rkm.auc << std::endl;
    }
    return 0;
}

int main(int argc, char *argv[])
{
    Job J;
    std::string fname, probename, mname, lname;
    bool balance = true;
    int K = 32, ngpu = getenv("BPMF_NGPU") ? atoi(getenv("BPMF_NGPU")) : 0;
    if (const char *e = getenv("BPMF_NUMLATENT")) K = atoi(e);

    bool fp32 = getenv("BPMF_HIP_F32") && atoi(getenv("BPMF_HIP_F32")) != 0;
    static const struct option long_opts[] = {{"fp32", no_argument, nullptr, 1000}, {"topn", required_argument, nullptr, 1001},
                                              {"topn-by", required_argument, nullptr, 1002}, {"noise", required_argument, nullptr, 1003},
                                              {"alpha-prior", required_argument, nullptr, 1004}, {"alpha-max", required_argument, nullptr, 1005},
                                              {"probit", no_argument, nullptr, 1006}, {"probit-threshold", required_argument, nullptr, 1007},
                                              {"row-features", required_argument, nullptr, 1008}, {"col-features", required_argument, nullptr, 1009},
                                              {"lambda-beta", required_argument, nullptr, 1010},
                                              {"link-tol", required_argument, nullptr, 1011}, {"link-max-iter", required_argument, nullptr, 1012},
                                              {"lambda-beta-prior", required_argument, nullptr, 1013},
                                              {"censored", required_argument, nullptr, 1014},
                                              {"weights", required_argument, nullptr, 1030}, {"robust", required_argument, nullptr, 1031},
                                              {"new-row-features", required_argument, nullptr, 1015}, {"new-col-features", required_argument, nullptr, 1016},
                                              {"topn-score", required_argument, nullptr, 1017}, {"topn-kappa", required_argument, nullptr, 1018},
                                              {"topn-threshold", required_argument, nullptr, 1019},
                                              {"fold-in-rows", required_argument, nullptr, 1020}, {"fold-in-cols", required_argument, nullptr, 1021},
                                              {"ordinal", no_argument, nullptr, 1050}, {"ordinal-levels", required_argument, nullptr, 1051},
                                              {"ordinal-cutpoints", required_argument, nullptr, 1052}, {"ordinal-step", required_argument, nullptr, 1053},
                                              {"tensor", required_argument, nullptr, 1040}, {"tensor-test", required_argument, nullptr, 1041},
                                              {"tensor-dims", required_argument, nullptr, 1042},
                                              {"implicit", required_argument, nullptr, 1060}, {"rank-eval", required_argument, nullptr, 1061},
                                              {"rank-by", required_argument, nullptr, 1062}, {"rank-threshold", required_argument, nullptr, 1063},
                                              {"save-model", required_argument, nullptr, 1070}, {"model", required_argument, nullptr, 1071},
                                              {"predict", required_argument, nullptr, 1072}, {"predict-threshold", required_argument, nullptr, 1073},
                                              {"similar", required_argument, nullptr, 1080}, {"similar-by", required_argument, nullptr, 1081},
                                              {"similar-kind", required_argument, nullptr, 1082}, {"similar-kappa", required_argument, nullptr, 1083},
                                              {"similar-min-ratings", required_argument, nullptr, 1084},
                                              {"bias", no_argument, nullptr, 1090}, {"bias-lambda", required_argument, nullptr, 1091},
                                              {"bias-prior", required_argument, nullptr, 1092},
                                              {"diagnose", no_argument, nullptr, 1100},
                                              {"score", no_argument, nullptr, 1101}, {"intervals", required_argument, nullptr, 1102},
                                              {"loo", no_argument, nullptr, 1103},
                                              {"chain", required_argument, nullptr, 1104}, {"diagnose-rank", no_argument, nullptr, 1105},
                                              {nullptr, 0, nullptr, 0}};
    std::string similar_n, similar_by = "cols", similar_kind = "cosine", similar_kappa, similar_min;
    std::string bias_lambda, bias_prior;
    bool bias_lambda_given = false, bias_prior_given = false;
    bool similar_given = false;
    std::string similar_flag;                                        // the first --similar-* flag given
    std::string topn_by = "rows", noise = "fixed", alpha_prior, alpha_max, probit_threshold, row_features, col_features, lambda_beta, link_tol, link_max_iter, lambda_beta_prior, censored_file, weights_file, robust_nu, new_row_features, new_col_features, fold_in_rows, fold_in_cols;
    std::string topn_score = "mean", topn_kappa, topn_threshold;
    bool topn_kappa_given = false, topn_threshold_given = false;
    bool alpha_given = false, threshold_given = false;
    std::string tensor_file, tensor_test, tensor_dims;
    std::string ordinal_levels, ordinal_cutpoints, ordinal_step;
    std::string implicit_w0, rank_eval_n, rank_by = "rows", rank_threshold;
    bool rank_eval_given = false, rank_by_given = false;
    std::string model_dir, predict_file, predict_threshold;
    std::string intervals;
    bool intervals_given = false;
    bool save_model_given = false, model_given = false, predict_given = false, predict_threshold_given = false;
    std::string chain_arg;
    bool chain_given = false;
    bool nsims_given = false, burnin_given = false, d_given = false, g_given = false;
    std::string training_flag;                                       // the first flag of the likelihood / the chain (refused with --model)
    auto training = [&](const char *flag) { if (training_flag.empty()) training_flag = flag; };
    bool ordinal_levels_given = false, ordinal_cutpoints_given = false;
    bool tensor_given = false, tensor_test_given = false, tensor_dims_given = false;
    int ch;
    while ((ch = getopt_long(argc, argv, "krvn:t:p:i:b:f:o:m:l:a:d:g:h", long_opts, nullptr)) != -1) {
        switch (ch) {
        case 1000: training("--fp32"); fp32 = true; break;
        case 1001: J.topn = atoi(optarg); if (J.topn < 1) die("--topn expects N >= 1"); break;
        case 1002: topn_by = optarg; break;
        case 1003: training("--noise"); noise = optarg; break;
        case 1004: training("--alpha-prior"); alpha_prior = optarg; break;
        case 1005: training("--alpha-max"); alpha_max = optarg; break;
        case 1006: training("--probit"); J.probit = true; break;
        case 1007: training("--probit-threshold"); probit_threshold = optarg; threshold_given = true; break;
        case 1008: training("--row-features"); row_features = optarg; break;
        case 1009: training("--col-features"); col_features = optarg; break;
        case 1010: training("--lambda-beta"); lambda_beta = optarg; break;
        case 1011: training("--link-tol"); link_tol = optarg; break;
        case 1012: training("--link-max-iter"); link_max_iter = optarg; break;
        case 1013: training("--lambda-beta-prior"); lambda_beta_prior = optarg; J.lb_sampled = true; break;
        case 1014: training("--censored"); censored_file = optarg; J.censored = true; break;
        case 1030: training("--weights"); weights_file = optarg; J.weighted = true; break;
        case 1031: training("--robust"); robust_nu = optarg; J.robust = true; break;
        case 1015: training("--new-row-features"); new_row_features = optarg; break;
        case 1016: training("--new-col-features"); new_col_features = optarg; break;
        case 1017: topn_score = optarg; break;
        case 1018: topn_kappa = optarg; topn_kappa_given = true; break;
        case 1019: topn_threshold = optarg; topn_threshold_given = true; break;
        case 1020: fold_in_rows = optarg; break;
        case 1021: fold_in_cols = optarg; break;
        case 1050: training("--ordinal"); J.ordinal = true; break;
        case 1051: training("--ordinal-levels"); ordinal_levels = optarg; ordinal_levels_given = true; break;
        case 1052: training("--ordinal-cutpoints"); ordinal_cutpoints = optarg; ordinal_cutpoints_given = true; break;
        case 1053: training("--ordinal-step"); ordinal_step = optarg; J.ord_step_given = true; break;
        case 1040: training("--tensor"); tensor_file = optarg; tensor_given = true; break;
        case 1041: training("--tensor-test"); tensor_test = optarg; tensor_test_given = true; break;
        case 1042: training("--tensor-dims"); tensor_dims = optarg; tensor_dims_given = true; break;
        case 1060: training("--implicit"); implicit_w0 = optarg; J.implicit = true; break;
        case 1061: rank_eval_n = optarg; rank_eval_given = true; break;
        case 1062: rank_by = optarg; rank_by_given = true; break;
        case 1063: rank_threshold = optarg; J.rank_thr_given = true; break;
        case 1070: J.save_model = optarg; save_model_given = true; break;
        case 1071: model_dir = optarg; model_given = true; break;
        case 1072: predict_file = optarg; predict_given = true; break;
        case 1073: predict_threshold = optarg; predict_threshold_given = true; break;
        case 1080: similar_n = optarg; similar_given = true; break;
        case 1081: similar_by = optarg; if (similar_flag.empty()) similar_flag = "--similar-by"; break;
        case 1082: similar_kind = optarg; if (similar_flag.empty()) similar_flag = "--similar-kind"; break;
        case 1083: similar_kappa = optarg; if (similar_flag.empty()) similar_flag = "--similar-kappa"; break;
        case 1084: similar_min = optarg; if (similar_flag.empty()) similar_flag = "--similar-min-ratings"; break;
        case 1090: training("--bias"); J.bias = true; break;
        case 1091: training("--bias-lambda"); bias_lambda = optarg; bias_lambda_given = true; break;
        case 1092: training("--bias-prior"); bias_prior = optarg; bias_prior_given = true; break;
        case 1100: J.diagnose = true; break;
        case 1101: J.score = true; break;
        case 1102: intervals = optarg; intervals_given = true; break;
        case 1103: J.loo = true; break;
        case 1104: training("--chain"); chain_arg = optarg; chain_given = true; break;
        case 1105: J.diagnose = true; J.diag_rank = true; break;
        case 'i': J.nsims = atoi(optarg); nsims_given = true; break;
        case 'b': J.burnin = atoi(optarg); burnin_given = true; break;
        case 'f': training("-f"); J.update_freq = atoi(optarg); break;
        case 't': training("-t"); J.nthrds = atoi(optarg); break;
        case 'a': J.alpha = atof(optarg); alpha_given = true; break;
        case 'd': K = atoi(optarg); d_given = true; break;
        case 'g': ngpu = atoi(optarg); g_given = true; break;
        case 'n': fname = optarg; break;
        case 'p': probename = optarg; break;
        case 'o': J.odirname = optarg; break;
        case 'm': training("-m"); mname = optarg; break;
        case 'l': training("-l"); lname = optarg; break;
        case 'r': training("-r"); J.redirect = true; break;
        case 'k': training("-k"); balance = false; break;
        case 'v': training("-v"); J.verbose = true; break;
        default: usage(); return 1;
        }
    }
    // --similar and its flags: refused before anything touches a GPU
    if (!similar_flag.empty() && !similar_given) die(similar_flag + " needs --similar N");
    if (similar_given) {
        char *end = nullptr;
        const long n = similar_n.empty() ? 0 : strtol(similar_n.c_str(), &end, 10);
        if (similar_n.empty() || *end != '\0' || n < 1 || n > 32) die("--similar expects 1 <= N <= 32, not '" + similar_n + "'");
        J.similar = (int)n;
        if (similar_by != "cols" && similar_by != "rows") die("--similar-by expects cols or rows, not '" + similar_by + "'");
        J.similar_by_rows = similar_by == "rows";
        if (similar_kind != "cosine" && similar_kind != "euclid") die("--similar-kind expects cosine or euclid, not '" + similar_kind + "'");
        J.similar_kind = similar_kind == "cosine" ? BPMF_HIP_SIM_COSINE : BPMF_HIP_SIM_EUCLID;
        if (!similar_kappa.empty() || similar_flag == "--similar-kappa") {
            J.similar_kappa = similar_kappa.empty() ? NAN : strtod(similar_kappa.c_str(), &end);
            if (similar_kappa.empty() || *end != '\0' || !std::isfinite(J.similar_kappa) || J.similar_kappa < 0.0)
                die("--similar-kappa expects a finite number >= 0, not '" + similar_kappa + "'");
        }
        if (!similar_min.empty() || similar_flag == "--similar-min-ratings") {
            J.similar_min = similar_min.empty() ? -1 : strtol(similar_min.c_str(), &end, 10);
            if (similar_min.empty() || *end != '\0' || J.similar_min < 0) die("--similar-min-ratings expects an integer >= 0, not '" + similar_min + "'");
        }
        if (tensor_given) die("--similar does not go together with --tensor (the similarity is between the columns of one side of a matrix)");
        if (g_given || ngpu >= 1) die("--similar runs on one GPU without -g: -g " + std::to_string(ngpu) + " is not supported (the sample ring of a sharded side is not complete)");
        if (getenv("BPMF_REDUCE") && atoi(getenv("BPMF_REDUCE")) != 0) die("--similar does not go together with BPMF_REDUCE=1");
        if (!mname.empty() || !lname.empty()) die("--similar does not go together with a propagated posterior (-m / -l)");
        if (J.odirname.empty()) die(std::string("--similar needs -o DIR (the lists go to DIR/similar-") + (J.similar_by_rows ? "rows" : "cols") + ".csv)");
        if (!model_given && J.nsims <= J.burnin) die("--similar needs at least one post-burn-in sample (-i > -b)");
        if (model_given && J.similar_min > 0 && fname.empty()) die("--similar-min-ratings with --model needs -n TRAIN (the training ratings are what it counts)");
    }
    // --diagnose: refused before anything touches a GPU
    if (J.diagnose) {
        if (tensor_given) die("--diagnose does not go together with --tensor (the diagnosed predictions are those of a matrix model)");
        if (g_given || ngpu >= 1) die("--diagnose runs on one GPU without -g: -g " + std::to_string(ngpu) + " is not supported (the sample ring of a sharded side is not complete)");
        if (getenv("BPMF_REDUCE") && atoi(getenv("BPMF_REDUCE")) != 0) die("--diagnose does not go together with BPMF_REDUCE=1");
        if (!mname.empty() || !lname.empty()) die("--diagnose does not go together with a propagated posterior (-m / -l)");
        if (model_given && !predict_given) die("--diagnose with --model needs --predict FILE (the cells whose predictions are diagnosed)");
        if (!model_given && (J.nsims - J.burnin < 8 || J.nsims - J.burnin > BPMF_HIP_DIAG_MAX_SAMPLES))
            die("--diagnose needs 8 .. " + std::to_string(BPMF_HIP_DIAG_MAX_SAMPLES) + " post-burn-in samples (-i - -b = " + std::to_string(J.nsims - J.burnin) + ")");
    }
    // --chain: refused before anything touches a GPU (the refusals of bpmf_hip_side_set_chain)
    if (chain_given) {
        char *end = nullptr;
        const long c = chain_arg.empty() ? -1 : strtol(chain_arg.c_str(), &end, 10);
        if (chain_arg.empty() || *end != '\0' || c < 0 || c > BPMF_HIP_CHAIN_MAX) die("--chain expects 0 <= c <= " + std::to_string(BPMF_HIP_CHAIN_MAX) + ", not '" + chain_arg + "'");
        J.chain = (int)c;
        if (tensor_given) die("--chain does not go together with --tensor");
        if (!row_features.empty() || !col_features.empty() || !new_row_features.empty() || !new_col_features.empty()) die("--chain does not go together with features (--row-features / --col-features)");
        if (J.ordinal) die("--chain does not go together with --ordinal");
        if (J.bias) die("--chain does not go together with --bias");
        if (J.implicit) die("--chain does not go together with --implicit");
        if (g_given || ngpu >= 1) die("--chain runs on one GPU without -g: -g " + std::to_string(ngpu) + " is not supported (run one process per chain and GPU)");
        if (getenv("BPMF_REDUCE") && atoi(getenv("BPMF_REDUCE")) != 0) die("--chain does not go together with BPMF_REDUCE=1");
        if (!mname.empty() || !lname.empty()) die("--chain does not go together with a propagated posterior (-m / -l)");
        if (J.nsims > BPMF_HIP_CHAIN_STRIDE) die("--chain needs -i <= " + std::to_string(BPMF_HIP_CHAIN_STRIDE) + " (the chains' random streams are that many half-iterations apart), not -i " + std::to_string(J.nsims));
    }
    // --score: refused before anything touches a GPU
    if (J.score) {
        if (tensor_given) die("--score does not go together with --tensor (the scored likelihoods are those of a matrix model)");
        if (J.ordinal) die("--score does not go together with --ordinal (its held-out log density is the `Final log-prob` line)");
        if (J.implicit) die("--score does not go together with --implicit (its likelihood runs over every cell of the matrix)");
        if (g_given || ngpu >= 1) die("--score runs on one GPU without -g: -g " + std::to_string(ngpu) + " is not supported (the sample ring of a sharded side is not complete)");
        if (getenv("BPMF_REDUCE") && atoi(getenv("BPMF_REDUCE")) != 0) die("--score does not go together with BPMF_REDUCE=1");
        if (!mname.empty() || !lname.empty()) die("--score does not go together with a propagated posterior (-m / -l)");
        if (model_given && !predict_given && fname.empty()) die("--score with --model needs --predict FILE (held-out cells with their values) or -n TRAIN (the cells of WAIC)");
        if (!model_given && J.nsims - J.burnin < 2) die("--score needs at least 2 post-burn-in samples (-i - -b = " + std::to_string(J.nsims - J.burnin) + ")");
    }
    // --loo: refused before anything touches a GPU
    if (J.loo) {
        if (tensor_given) die("--loo does not go together with --tensor (the scored likelihoods are those of a matrix model)");
        if (J.ordinal) die("--loo does not go together with --ordinal (its likelihood over levels is not among the scored ones)");
        if (J.implicit) die("--loo does not go together with --implicit (its likelihood runs over every cell of the matrix)");
        if (g_given || ngpu >= 1) die("--loo runs on one GPU without -g: -g " + std::to_string(ngpu) + " is not supported (the sample ring of a sharded side is not complete)");
        if (getenv("BPMF_REDUCE") && atoi(getenv("BPMF_REDUCE")) != 0) die("--loo does not go together with BPMF_REDUCE=1");
        if (!mname.empty() || !lname.empty()) die("--loo does not go together with a propagated posterior (-m / -l)");
        if (model_given && fname.empty()) die("--loo with --model needs -n TRAIN (the training cells are what is cross-validated)");
        if (!model_given && (J.nsims - J.burnin < 2 || J.nsims - J.burnin > BPMF_HIP_LOO_MAX_SAMPLES))
            die("--loo needs 2 .. " + std::to_string(BPMF_HIP_LOO_MAX_SAMPLES) + " post-burn-in samples (-i - -b = " + std::to_string(J.nsims - J.burnin) + ")");
    }
    // --intervals: refused before anything touches a GPU
    if (intervals_given) {
        const std::string expects = "--intervals expects 1 .. 4 distinct levels in [0.01, 0.998] separated by commas, not '" + intervals + "'";
        for (size_t from = 0; from <= intervals.size();) {
            const size_t to = std::min(intervals.find(',', from), intervals.size());
            const std::string word = intervals.substr(from, to - from);
            char *e = nullptr;
            const double l = strtod(word.c_str(), &e);
            if (word.empty() || *e != '\0' || !(l >= 0.01 && l <= 0.998) || J.iv_levels.size() == 4) die(expects);
            for (double have : J.iv_levels) if (have == l) die(expects);
            J.iv_levels.push_back(l);
            from = to + 1;
        }
        for (double l : J.iv_levels) { J.iv_tau.push_back((1.0 - l) / 2.0); J.iv_tau.push_back((1.0 + l) / 2.0); }
        std::sort(J.iv_tau.begin(), J.iv_tau.end());
        for (double l : J.iv_levels) {
            J.iv_lo.push_back((int)(std::find(J.iv_tau.begin(), J.iv_tau.end(), (1.0 - l) / 2.0) - J.iv_tau.begin()));
            J.iv_hi.push_back((int)(std::find(J.iv_tau.begin(), J.iv_tau.end(), (1.0 + l) / 2.0) - J.iv_tau.begin()));
        }
        if (tensor_given) die("--intervals does not go together with --tensor (the intervals are those of a matrix model)");
        if (J.ordinal) die("--intervals does not go together with --ordinal (its predictive is over levels)");
        if (J.probit) die("--intervals does not go together with --probit (its predictive is a probability, not an interval)");
        if (J.implicit) die("--intervals does not go together with --implicit (its likelihood runs over every cell of the matrix)");
        if (J.robust) die("--intervals does not go together with --robust (a mixture of Student-t distributions needs an incomplete beta function on the device: deliberately out of scope)");
        if (g_given || ngpu >= 1) die("--intervals runs on one GPU without -g: -g " + std::to_string(ngpu) + " is not supported (the sample ring of a sharded side is not complete)");
        if (getenv("BPMF_REDUCE") && atoi(getenv("BPMF_REDUCE")) != 0) die("--intervals does not go together with BPMF_REDUCE=1");
        if (!mname.empty() || !lname.empty()) die("--intervals does not go together with a propagated posterior (-m / -l)");
        if (model_given && !predict_given) die("--intervals with --model needs --predict FILE (the cells, with their values as the observations)");
        if (!model_given && probename.empty()) die("--intervals needs a test matrix (-p TEST: its cells get the intervals, its values the calibration)");
        if (!model_given && (J.nsims - J.burnin < 1 || J.nsims - J.burnin > BPMF_HIP_INTERVAL_MAX_SAMPLES))
            die("--intervals needs 1 .. " + std::to_string(BPMF_HIP_INTERVAL_MAX_SAMPLES) + " post-burn-in samples (-i - -b = " + std::to_string(J.nsims - J.burnin) + ")");
    }
    // --model / --predict / --save-model: refused before anything touches a GPU
    if (predict_given && !model_given) die("--predict needs --model DIR (cells are predicted from a saved model)");
    if (predict_threshold_given && !predict_given) die("--predict-threshold needs --predict FILE");
    double predict_thr = 0.0;
    if (predict_threshold_given) {
        char *e = nullptr;
        predict_thr = strtod(predict_threshold.c_str(), &e);
        if (e == predict_threshold.c_str() || *e != '\0' || !std::isfinite(predict_thr)) die("--predict-threshold expects a finite number, not '" + predict_threshold + "'");
    }
    if (model_given) {
        if (model_dir.empty()) die("--model expects a directory");
        if (save_model_given) die("--model does not go together with --save-model (no chain runs)");
        if (nsims_given || burnin_given) die(std::string("--model does not go together with ") + (nsims_given ? "-i" : "-b") + " (no chain runs)");
        if (alpha_given) die("--model does not go together with -a (the model has its alpha)");
        if (g_given || ngpu >= 1) die("--model runs on one GPU without -g");
        if (!training_flag.empty()) die("--model does not go together with " + training_flag + " (no chain runs; the likelihood is the model's)");
        if (getenv("BPMF_REDUCE") && atoi(getenv("BPMF_REDUCE")) != 0) die("--model does not go together with BPMF_REDUCE=1");
        if (predict_given && predict_file.empty()) die("--predict expects a file");
        if (J.topn > 0 && fname.empty()) die("--topn with --model needs -n TRAIN (the rated cells are what the lists exclude)");
        if (rank_eval_given && fname.empty()) die("--rank-eval with --model needs -n TRAIN (the rated cells are what the ranks exclude)");
        if (rank_eval_given && probename.empty()) die("--rank-eval with --model needs -p TEST (the held-out cells)");
        if (!predict_given && J.topn < 1 && !rank_eval_given && fold_in_rows.empty() && fold_in_cols.empty() && !similar_given && !J.score && !J.loo)
            die("--model: nothing to do (--predict FILE, --topn N, --rank-eval N, --similar N, --fold-in-rows FILE or --fold-in-cols FILE)");
        if (J.odirname.empty()) die("--model needs -o DIR (the results go to files in DIR)");
    }
    if (save_model_given) {
        if (J.save_model.empty()) die("--save-model expects a directory");
        if (tensor_given) die("--save-model does not go together with --tensor (model format 1 stores two sides)");
        if (g_given || ngpu >= 1) die("--save-model runs on one GPU without -g: -g " + std::to_string(ngpu) + " is not supported (the sample rings of a sharded side are not complete)");
        if (getenv("BPMF_REDUCE") && atoi(getenv("BPMF_REDUCE")) != 0) die("--save-model does not go together with BPMF_REDUCE=1");
        if (J.ordinal) die("--save-model does not go together with --ordinal (model format 1 does not store the cutpoints)");
        if (J.implicit) die("--save-model does not go together with --implicit (model format 1 does not store the Gram matrix)");
        if (!row_features.empty() || !col_features.empty()) die("--save-model does not go together with --row-features / --col-features (model format 1 does not store the link matrix per sample)");
        if (!mname.empty() || !lname.empty()) die("--save-model does not go together with a propagated posterior (-m / -l)");
        if (J.nsims <= J.burnin) die("--save-model needs at least one post-burn-in sample (-i > -b)");
    }
    // --tensor: refused before anything touches a GPU, then a loop of its own (run_tensor)
    if ((tensor_test_given || tensor_dims_given) && !tensor_given) die(std::string(tensor_test_given ? "--tensor-test" : "--tensor-dims") + " needs --tensor FILE.tns");
    if (tensor_given) {
        if (tensor_file.empty()) die("--tensor expects a file");
        if (!fname.empty() || !probename.empty()) die("--tensor takes the place of the matrix files: -n / -p do not go together with it");
        if (ngpu >= 1) die("--tensor runs on one GPU without -g: -g " + std::to_string(ngpu) + " is not supported (a mode's side is not sharded)");
        if (fp32) die("--tensor does not go together with --fp32 (the Khatri-Rao rows and their samplers are fp64)");
        if (!mname.empty() || !lname.empty()) die("--tensor does not go together with a propagated posterior (-m / -l)");
        if (getenv("BPMF_REDUCE") && atoi(getenv("BPMF_REDUCE")) != 0) die("--tensor does not go together with BPMF_REDUCE=1");
        if (J.probit || threshold_given) die("--tensor does not go together with --probit");
        if (J.ordinal || ordinal_levels_given || ordinal_cutpoints_given || J.ord_step_given) die("--tensor does not go together with --ordinal");
        if (J.censored) die("--tensor does not go together with --censored");
        if (J.weighted) die("--tensor does not go together with --weights");
        if (J.robust) die("--tensor does not go together with --robust");
        if (J.bias) die("--tensor does not go together with --bias");
        if (J.implicit) die("--implicit does not go together with --tensor (a mode's side is a plain Gaussian side)");
        if (rank_eval_given || rank_by_given || J.rank_thr_given) die("--tensor does not go together with --rank-eval");
        if (noise != "fixed" || !alpha_prior.empty() || !alpha_max.empty()) die("--tensor does not go together with --noise adaptive");
        if (!row_features.empty() || !col_features.empty() || !new_row_features.empty() || !new_col_features.empty() || !lambda_beta.empty() ||
            !lambda_beta_prior.empty() || !link_tol.empty() || !link_max_iter.empty())
            die("--tensor does not go together with --row-features / --col-features");
        if (J.topn > 0 || topn_score != "mean" || topn_kappa_given || topn_threshold_given) die("--tensor does not go together with --topn");
        if (!fold_in_rows.empty() || !fold_in_cols.empty()) die("--tensor does not go together with --fold-in-rows / --fold-in-cols");
        if (J.verbose) die("--tensor does not go together with -v");
        if (!bpmf_hip_supports(K, BPMF_HIP_F64)) die("unsupported number of latent dimensions " + std::to_string(K) + " (1 .. 128)");
        if (!(J.alpha > 0.0) || !std::isfinite(J.alpha)) die("--tensor needs a noise precision -a F > 0");
        return run_tensor(tensor_file, tensor_test, tensor_dims, tensor_dims_given, K, J.nsims, J.burnin, J.alpha, J.odirname);
    }
    if (!model_given && (fname.empty() || probename.empty())) { usage(); return 1; }
    // --topn: checked before anything touches a GPU
    if (topn_by != "rows" && topn_by != "cols") die("--topn-by expects rows or cols, not '" + topn_by + "'");
    J.topn_by_cols = topn_by == "cols";
    if (J.topn > 0) {
        if (J.odirname.empty()) die("--topn needs -o DIR (the lists go to DIR/topn.csv)");
        if (ngpu > 1) die("--topn runs on one GPU: -g " + std::to_string(ngpu) + " is not supported (the sharded replicas are not complete on every rank)");
        if (J.topn > 32) die("--topn expects 1 <= N <= 32");
        if (J.nsims <= J.burnin) die("--topn needs at least one post-burn-in sample (-i > -b)");
    }
    // --noise / --alpha-prior / --alpha-max: checked before anything touches a GPU
    if (noise != "fixed" && noise != "adaptive") die("--noise expects fixed or adaptive, not '" + noise + "'");
    J.adaptive = noise == "adaptive";
    // --topn-score / --topn-kappa / --topn-threshold: checked before anything touches a GPU
    {
        if (topn_score != "mean" && topn_score != "ucb" && topn_score != "prob" && topn_score != "ei")
            die("--topn-score expects mean, ucb, prob or ei, not '" + topn_score + "'");
        const bool ucb = topn_score == "ucb", thr = topn_score == "prob" || topn_score == "ei";
        if (topn_score != "mean" && J.topn < 1) die("--topn-score " + topn_score + " needs --topn N (it ranks the top-N lists)");
        if (topn_kappa_given && !ucb) die("--topn-kappa goes with --topn-score ucb only");
        if (topn_threshold_given && !thr) die("--topn-threshold goes with --topn-score prob or ei only");
        auto number = [&](const std::string &text, const char *flag) {
            char *e = nullptr;
            const double v = strtod(text.c_str(), &e);
            if (e == text.c_str() || *e != '\0' || !std::isfinite(v)) die(std::string(flag) + " expects a finite number, not '" + text + "'");
            return v;
        };
        if (thr && !topn_threshold_given) die("--topn-score " + topn_score + " needs --topn-threshold F");
        if (thr && J.adaptive) die("--topn-score " + topn_score + " does not go together with --noise adaptive (alpha is not a single number, and sigma = 1 / sqrt(alpha) is part of the score)");
        if (topn_score != "mean" && (!new_row_features.empty() || !new_col_features.empty()))
            die("--topn-score " + topn_score + " does not go together with --new-row-features / --new-col-features (their lists are ranked by the mean)");
        if (ucb) { J.topn_kind = BPMF_HIP_SCORE_UCB; J.topn_param = topn_kappa_given ? number(topn_kappa, "--topn-kappa") : 1.0; }
        if (thr) {
            J.topn_kind = topn_score == "prob" ? BPMF_HIP_SCORE_PROB : BPMF_HIP_SCORE_EI;
            J.topn_param = number(topn_threshold, "--topn-threshold");
            if (!J.probit && !J.ordinal && !(J.alpha > 0.0 && std::isfinite(J.alpha))) die("--topn-score " + topn_score + " needs a finite -a > 0 (sigma = 1 / sqrt(alpha))");
            J.topn_sigma = (J.probit || J.ordinal) ? 1.0 : 1.0 / std::sqrt(J.alpha);
        }
    }
    if (!J.adaptive && (!alpha_prior.empty() || !alpha_max.empty())) die("--alpha-prior and --alpha-max need --noise adaptive");
    if (J.adaptive) {
        if (!alpha_prior.empty()) {
            const char *s0 = alpha_prior.c_str();
            char *e1 = nullptr, *e2 = nullptr;
            J.a0 = strtod(s0, &e1);
            if (e1 == s0 || *e1 != ',') die("--alpha-prior expects A0,B0, not '" + alpha_prior + "'");
            J.b0 = strtod(e1 + 1, &e2);
            if (e2 == e1 + 1 || *e2 != '\0') die("--alpha-prior expects A0,B0, not '" + alpha_prior + "'");
            if (!(J.a0 > 0.0) || !(J.b0 >= 0.0) || !std::isfinite(J.a0) || !std::isfinite(J.b0))
                die("--alpha-prior expects a shape A0 > 0 and a rate B0 >= 0, not '" + alpha_prior + "'");
        }
        if (!alpha_max.empty()) {
            char *e = nullptr;
            J.alpha_max = strtod(alpha_max.c_str(), &e);
            if (e == alpha_max.c_str() || *e != '\0' || !(J.alpha_max > 0.0) || !std::isfinite(J.alpha_max))
                die("--alpha-max expects a number F > 0, not '" + alpha_max + "'");
        }
        if (ngpu >= 1) die("--noise adaptive runs on one GPU without -g: -g " + std::to_string(ngpu) + " is not supported (the sum of the "
                           "training residuals is not all-reduced over ranks)");
        if (!(J.alpha > 0.0)) die("--noise adaptive needs an initial alpha -a F > 0");
    }
    // --probit / --probit-threshold: checked before anything touches a GPU
    if (threshold_given && !J.probit) die("--probit-threshold needs --probit");
    if (J.probit) {
        if (threshold_given) {
            char *e = nullptr;
            J.probit_threshold = strtod(probit_threshold.c_str(), &e);
            if (e == probit_threshold.c_str() || *e != '\0' || !std::isfinite(J.probit_threshold))
                die("--probit-threshold expects a number, not '" + probit_threshold + "'");
        }
        if (J.adaptive) die("--probit does not go together with --noise adaptive (the latent scores have unit variance)");
        if (ngpu >= 1) die("--probit runs on one GPU without -g: -g " + std::to_string(ngpu) + " is not supported (the latent scores of a "
                           "sharded side are not drawn)");
        if (getenv("BPMF_REDUCE") && atoi(getenv("BPMF_REDUCE")) != 0) die("--probit does not go together with BPMF_REDUCE=1");
        if (alpha_given && J.alpha != 1.0) die("--probit runs with alpha = 1: -a " + std::to_string(J.alpha) + " is not supported");
        J.alpha = 1.0;
    }
    // --ordinal / --ordinal-levels / --ordinal-cutpoints / --ordinal-step: checked before anything touches a GPU (the values of the
    // matrices below, once they are read)
    if ((ordinal_levels_given || ordinal_cutpoints_given || J.ord_step_given) && !J.ordinal)
        die(std::string(ordinal_levels_given ? "--ordinal-levels" : ordinal_cutpoints_given ? "--ordinal-cutpoints" : "--ordinal-step") + " needs --ordinal");
    if (J.ordinal) {
        auto number_list = [&](const std::string &text, const char *flag) {
            std::vector<double> v;
            const char *p = text.c_str();
            for (;;) {
                char *e = nullptr;
                const double x = strtod(p, &e);
                if (e == p || !std::isfinite(x) || (*e != ',' && *e != '\0')) die(std::string(flag) + " expects finite numbers separated by commas, not '" + text + "'");
                v.push_back(x);
                if (*e == '\0') break;
                p = e + 1;
            }
            for (size_t k = 1; k < v.size(); ++k) if (!(v[k] > v[k - 1])) die(std::string(flag) + " expects strictly increasing numbers, not '" + text + "'");
            return v;
        };
        if (ordinal_levels_given) {
            J.ord_levels = number_list(ordinal_levels, "--ordinal-levels");
            if (J.ord_levels.size() < 2 || J.ord_levels.size() > 16) die("--ordinal-levels expects 2 .. 16 levels, not " + std::to_string(J.ord_levels.size()));
        }
        if (ordinal_cutpoints_given) {
            J.ord_cut0 = number_list(ordinal_cutpoints, "--ordinal-cutpoints");
            J.ord_fixed = true;
            if (ordinal_levels_given && J.ord_cut0.size() + 1 != J.ord_levels.size())
                die("--ordinal-cutpoints expects " + std::to_string(J.ord_levels.size() - 1) + " cutpoints for " + std::to_string(J.ord_levels.size()) + " levels");
        }
        if (J.ord_step_given) {
            char *e = nullptr;
            J.ord_step = strtod(ordinal_step.c_str(), &e);
            if (e == ordinal_step.c_str() || *e != '\0' || !std::isfinite(J.ord_step) || !(J.ord_step > 0.0))
                die("--ordinal-step expects a number F > 0, not '" + ordinal_step + "'");
            if (J.ord_fixed) die("--ordinal-step does not go together with --ordinal-cutpoints (fixed cutpoints are not proposed)");
        }
        if (J.probit || threshold_given) die("--ordinal does not go together with --probit (a side has one likelihood)");
        if (J.adaptive) die("--ordinal does not go together with --noise adaptive (the latent scores have unit variance)");
        if (ngpu >= 1) die("--ordinal runs on one GPU without -g: -g " + std::to_string(ngpu) + " is not supported (the latent scores of a "
                           "sharded side are not drawn)");
        if (getenv("BPMF_REDUCE") && atoi(getenv("BPMF_REDUCE")) != 0) die("--ordinal does not go together with BPMF_REDUCE=1");
        if (alpha_given && J.alpha != 1.0) die("--ordinal runs with alpha = 1: -a " + std::to_string(J.alpha) + " is not supported");
        if (!mname.empty() || !lname.empty()) die("--ordinal does not go together with a propagated posterior (-m / -l)");
        if (!row_features.empty() || !col_features.empty()) die("--ordinal does not go together with --row-features / --col-features");
        if (J.censored) die("--ordinal does not go together with --censored (levels have no bounds)");
        if (J.weighted) die("--ordinal does not go together with --weights (the latent scores have unit variance)");
        if (J.robust) die("--ordinal does not go together with --robust (the latent scores have unit variance)");
        if (!fold_in_rows.empty() || !fold_in_cols.empty())
            die("--ordinal does not go together with --fold-in-rows / --fold-in-cols (levels would need a latent iteration of their own)");
        J.alpha = 1.0;
    }
    // --row-features / --col-features / --lambda-beta: checked before anything touches a GPU
    const bool linked = !row_features.empty() || !col_features.empty();
    if (!lambda_beta.empty() && !linked) die("--lambda-beta needs --row-features or --col-features");
    if (J.lb_sampled) {
        if (!linked) die("--lambda-beta-prior needs --row-features or --col-features");
        const char *s0 = lambda_beta_prior.c_str();
        char *e1 = nullptr, *e2 = nullptr;
        J.lb_a0 = strtod(s0, &e1);
        if (e1 == s0 || *e1 != ',') die("--lambda-beta-prior expects A0,B0, not '" + lambda_beta_prior + "'");
        J.lb_b0 = strtod(e1 + 1, &e2);
        if (e2 == e1 + 1 || *e2 != '\0') die("--lambda-beta-prior expects A0,B0, not '" + lambda_beta_prior + "'");
        if (!(J.lb_a0 > 0.0) || !(J.lb_b0 >= 0.0) || !std::isfinite(J.lb_a0) || !std::isfinite(J.lb_b0))
            die("--lambda-beta-prior expects a shape A0 > 0 and a rate B0 >= 0, not '" + lambda_beta_prior + "'");
    }
    auto sparse_file = [](const std::string &name) {
        if (name.empty()) return false;
        const bpmf::io::FileType ft = bpmf::io::file_type(name);
        if (ft.kind == bpmf::io::Kind::sdm || ft.kind == bpmf::io::Kind::sbm) return true;
        return ft.kind == bpmf::io::Kind::mtx && bpmf::io::mtx_is_coordinate(name);
    };
    const bool sparse_u = sparse_file(row_features), sparse_m = sparse_file(col_features);
    // --new-row-features / --new-col-features: checked before anything touches a GPU
    auto check_new = [&](const std::string &name, const std::string &have, bool have_sparse, const char *what, const char *partner) {
        if (name.empty()) return;
        const std::string w = std::string("--") + what;
        if (have.empty()) die(w + " needs --" + partner + " (the link matrix is fitted on the features of the training matrix)");
        if (J.odirname.empty()) die(w + " needs -o DIR (the predictions go to files in DIR)");
        if (J.nsims <= J.burnin) die(w + " needs at least one post-burn-in sample (-i > -b)");
        if (sparse_file(name) != have_sparse)
            die(w + ": " + name + " is " + (have_sparse ? "dense" : "sparse") + ", --" + partner + " " + have + " is " + (have_sparse ? "sparse" : "dense") +
                " (both files must be of the same kind)");
    };
    check_new(new_row_features, row_features, sparse_u, "new-row-features", "row-features");
    check_new(new_col_features, col_features, sparse_m, "new-col-features", "col-features");
    if ((!link_tol.empty() || !link_max_iter.empty()) && !sparse_u && !sparse_m)
        die("--link-tol / --link-max-iter need a sparse feature file (--row-features / --col-features FILE.sdm, .sbm or a coordinate .mtx)");
    if (!link_tol.empty()) {
        char *e = nullptr;
        J.link_tol = strtod(link_tol.c_str(), &e);
        if (e == link_tol.c_str() || *e != '\0' || !(J.link_tol > 0.0) || !(J.link_tol < 1.0)) die("--link-tol expects a number 0 < F < 1, not '" + link_tol + "'");
    }
    if (!link_max_iter.empty()) {
        char *e = nullptr;
        const long v = strtol(link_max_iter.c_str(), &e, 10);
        if (e == link_max_iter.c_str() || *e != '\0' || v < 1 || v > 1000000) die("--link-max-iter expects an integer 1 .. 1000000, not '" + link_max_iter + "'");
        J.link_max_iter = (int)v;
    }
    if (linked) {
        if (!lambda_beta.empty()) {
            char *e = nullptr;
            J.lambda_beta = strtod(lambda_beta.c_str(), &e);
            if (e == lambda_beta.c_str() || *e != '\0' || !std::isfinite(J.lambda_beta) || !(J.lambda_beta > 0.0))
                die("--lambda-beta expects a number F > 0, not '" + lambda_beta + "'");
        }
        if (ngpu >= 1) die("--row-features / --col-features run on one GPU without -g: -g " + std::to_string(ngpu) + " is not supported (the "
                           "products over the features of a sharded side are not formed)");
        if (J.probit) die("--row-features / --col-features do not go together with --probit");
        if (J.adaptive) die("--row-features / --col-features do not go together with --noise adaptive");
        if (fp32) die("--row-features / --col-features do not go together with --fp32 (the link is fp64)");
        if (!mname.empty() || !lname.empty()) die("--row-features / --col-features do not go together with a propagated posterior (-m / -l)");
        if (getenv("BPMF_REDUCE") && atoi(getenv("BPMF_REDUCE")) != 0) die("--row-features / --col-features do not go together with BPMF_REDUCE=1");
    }
    // --censored: checked before anything touches a GPU (the file itself below, once the training matrix is read)
    if (J.censored) {
        if (censored_file.empty()) die("--censored expects a file");
        if (ngpu >= 1) die("--censored runs on one GPU without -g: -g " + std::to_string(ngpu) + " is not supported (the latent values of a "
                           "sharded side are not drawn)");
        if (J.probit) die("--censored does not go together with --probit (labels have no bounds)");
        if (J.adaptive) die("--censored does not go together with --noise adaptive (alpha | y needs a fresh draw of every censored value from "
                            "the newest factors of both sides)");
        if (linked) die("--censored does not go together with --row-features / --col-features (the residuals would have to be formed from the "
                        "latent values)");
        if (!mname.empty() || !lname.empty()) die("--censored does not go together with a propagated posterior (-m / -l)");
        if (getenv("BPMF_REDUCE") && atoi(getenv("BPMF_REDUCE")) != 0) die("--censored does not go together with BPMF_REDUCE=1");
        if (!(J.alpha > 0.0) || !std::isfinite(J.alpha)) die("--censored needs a noise precision -a F > 0");
    }
    // --weights: checked before anything touches a GPU (the file itself below, once the training matrix is read)
    if (J.weighted) {
        if (weights_file.empty()) die("--weights expects a file");
        if (ngpu >= 1) die("--weights runs on one GPU without -g: -g " + std::to_string(ngpu) + " is not supported (a sharded side has no weighted sampler)");
        if (J.probit) die("--weights does not go together with --probit (the latent scores have unit variance)");
        if (J.censored) die("--weights does not go together with --censored (the latent draw would need the weight of its cell)");
        if (J.adaptive) die("--weights does not go together with --noise adaptive (alpha | r would need the weighted residuals)");
        if (linked) die("--weights does not go together with --row-features / --col-features (the link matrix would need the weighted residuals)");
        if (!mname.empty() || !lname.empty()) die("--weights does not go together with a propagated posterior (-m / -l)");
        if (fp32) die("--weights does not go together with --fp32 (the weighted samplers are fp64)");
        if (getenv("BPMF_REDUCE") && atoi(getenv("BPMF_REDUCE")) != 0) die("--weights does not go together with BPMF_REDUCE=1");
        if (!sparse_file(weights_file)) die("--weights: " + weights_file + " is not a sparse matrix file (.sdm or a coordinate .mtx)");
    }
    // --robust: checked before anything touches a GPU
    if (J.robust) {
        char *end = nullptr;
        J.robust_nu = robust_nu.empty() ? NAN : strtod(robust_nu.c_str(), &end);
        if (robust_nu.empty() || *end != '\0' || !std::isfinite(J.robust_nu) || !(J.robust_nu >= 1.0))
            die("--robust expects the degrees of freedom NU, a finite number >= 1, not '" + robust_nu + "'");
        if (ngpu >= 1) die("--robust runs on one GPU without -g: -g " + std::to_string(ngpu) + " is not supported (a sharded side has no weighted sampler)");
        if (J.weighted) die("--robust does not go together with --weights (the weights of Student-t noise are redrawn in every half-iteration)");
        if (J.probit) die("--robust does not go together with --probit (the latent scores have unit variance)");
        if (J.censored) die("--robust does not go together with --censored (the latent draw would need the weight of its cell)");
        if (J.adaptive) die("--robust does not go together with --noise adaptive (alpha | r would need the weighted residuals)");
        if (linked) die("--robust does not go together with --row-features / --col-features (the link matrix would need the weighted residuals)");
        if (!mname.empty() || !lname.empty()) die("--robust does not go together with a propagated posterior (-m / -l)");
        if (fp32) die("--robust does not go together with --fp32 (the weighted samplers are fp64)");
        if (topn_score == "prob" || topn_score == "ei")
            die("--robust does not go together with --topn-score " + topn_score + " (its sigma = 1 / sqrt(alpha) assumes Gaussian noise; mean and ucb are fine)");
        if (getenv("BPMF_REDUCE") && atoi(getenv("BPMF_REDUCE")) != 0) die("--robust does not go together with BPMF_REDUCE=1");
        if (!(J.alpha > 0.0) || !std::isfinite(J.alpha)) die("--robust needs a noise precision -a F > 0");
    }
    // --bias: checked before anything touches a GPU
    if ((bias_lambda_given || bias_prior_given) && !J.bias) die(std::string(bias_lambda_given ? "--bias-lambda" : "--bias-prior") + " needs --bias");
    if (J.bias) {
        if (bias_prior_given) {
            char *e1 = nullptr, *e2 = nullptr;
            const size_t comma = bias_prior.find(',');
            const std::string sa = bias_prior.substr(0, comma), sb = comma == std::string::npos ? "" : bias_prior.substr(comma + 1);
            J.bias_a0 = sa.empty() ? NAN : strtod(sa.c_str(), &e1);
            J.bias_b0 = sb.empty() ? NAN : strtod(sb.c_str(), &e2);
            if (sa.empty() || sb.empty() || *e1 != '\0' || *e2 != '\0' || !std::isfinite(J.bias_a0) || !(J.bias_a0 > 0.0) || !std::isfinite(J.bias_b0) || !(J.bias_b0 >= 0.0))
                die("--bias-prior expects A0,B0 with a finite A0 > 0 and a finite B0 >= 0, not '" + bias_prior + "'");
            J.bias_sampled = true;
        }
        if (bias_lambda_given) {
            char *end = nullptr;
            J.bias_lambda = bias_lambda.empty() ? NAN : strtod(bias_lambda.c_str(), &end);
            if (bias_lambda.empty() || *end != '\0' || !std::isfinite(J.bias_lambda) || !(J.bias_lambda > 0.0))
                die("--bias-lambda expects the precision of the bias prior, a finite number > 0, not '" + bias_lambda + "'");
        }
        if (ngpu >= 1) die("--bias runs on one GPU without -g: -g " + std::to_string(ngpu) + " is not supported (the bias step needs both sides whole)");
        if (J.probit) die("--bias does not go together with --probit (a side has one latent step)");
        if (J.ordinal) die("--bias does not go together with --ordinal (a side has one latent step)");
        if (J.censored) die("--bias does not go together with --censored (a side has one latent step)");
        if (J.robust) die("--bias does not go together with --robust (a side has one latent step)");
        if (J.weighted) die("--bias does not go together with --weights (the bias conditional is unweighted)");
        if (J.implicit) die("--bias does not go together with --implicit (the bias conditional would run over every cell)");
        if (tensor_given) die("--bias does not go together with --tensor");
        if (J.adaptive) die("--bias does not go together with --noise adaptive (the training residuals leave the biases out)");
        if (linked || !new_row_features.empty() || !new_col_features.empty())
            die("--bias does not go together with --row-features / --col-features (the residuals would have to be formed from the bias-free values)");
        if (!fold_in_rows.empty() || !fold_in_cols.empty()) die("--bias does not go together with --fold-in-rows / --fold-in-cols (a folded-in row would need a bias of its own)");
        if (save_model_given || model_given) die("--bias does not go together with --save-model / --model (the model format stores no biases)");
        if (similar_given) die("--bias does not go together with --similar (the two bias rows of the sample ring would enter the cosine)");
        if ((J.topn > 0 || rank_eval_given) && K > 126) die("--bias with --topn / --rank-eval needs -d <= 126 (the sample rings keep two more rows per sample)");
        if (!mname.empty() || !lname.empty()) die("--bias does not go together with a propagated posterior (-m / -l)");
        if (fp32) die("--bias does not go together with --fp32 (the bias kernels are fp64)");
        if (getenv("BPMF_REDUCE") && atoi(getenv("BPMF_REDUCE")) != 0) die("--bias does not go together with BPMF_REDUCE=1");
        if (!(J.alpha > 0.0) || !std::isfinite(J.alpha)) die("--bias needs a noise precision -a F > 0");
    }
    // --implicit: checked before anything touches a GPU (the confidences below, once --weights FILE is read)
    if (J.implicit) {
        char *end = nullptr;
        J.implicit_w0 = implicit_w0.empty() ? NAN : strtod(implicit_w0.c_str(), &end);
        if (implicit_w0.empty() || *end != '\0' || !std::isfinite(J.implicit_w0) || !(J.implicit_w0 > 0.0))
            die("--implicit expects the weight W0 of an unobserved cell, a finite number > 0, not '" + implicit_w0 + "'");
        if (ngpu >= 1) die("--implicit runs on one GPU without -g: -g " + std::to_string(ngpu) + " is not supported (the Gram matrix needs the other side whole)");
        if (fp32) die("--implicit does not go together with --fp32 (the weighted samplers are fp64)");
        if (J.probit) die("--implicit does not go together with --probit (a side has one likelihood)");
        if (J.ordinal) die("--implicit does not go together with --ordinal (a side has one likelihood)");
        if (J.robust) die("--implicit does not go together with --robust (the weights of Student-t noise are redrawn in every half-iteration)");
        if (J.censored) die("--implicit does not go together with --censored (the latent draw would need the confidence of its cell)");
        if (J.adaptive) die("--implicit does not go together with --noise adaptive (alpha | r would need the residuals of every cell)");
        if (linked) die("--implicit does not go together with --row-features / --col-features (the link matrix would need the weighted residuals)");
        if (!mname.empty() || !lname.empty()) die("--implicit does not go together with a propagated posterior (-m / -l)");
        if (!fold_in_rows.empty() || !fold_in_cols.empty()) die("--implicit does not go together with --fold-in-rows / --fold-in-cols (a folded-in row would need the Gram matrix)");
        if (topn_score == "prob" || topn_score == "ei")
            die("--implicit does not go together with --topn-score " + topn_score + " (its sigma = 1 / sqrt(alpha) is not the noise of a cell; mean and ucb are fine)");
        if (getenv("BPMF_REDUCE") && atoi(getenv("BPMF_REDUCE")) != 0) die("--implicit does not go together with BPMF_REDUCE=1");
        if (!(J.alpha > 0.0) || !std::isfinite(J.alpha)) die("--implicit needs a noise precision -a F > 0");
        if (!J.weighted && !(1.0 > J.implicit_w0)) die("--implicit " + implicit_w0 + ": without --weights every observed cell has the confidence 1, which is not > W0");
    }
    // --rank-eval / --rank-by / --rank-threshold: checked before anything touches a GPU
    if ((rank_by_given || J.rank_thr_given) && !rank_eval_given) die(std::string(rank_by_given ? "--rank-by" : "--rank-threshold") + " needs --rank-eval N");
    if (rank_eval_given) {
        char *end = nullptr;
        const long n = rank_eval_n.empty() ? 0 : strtol(rank_eval_n.c_str(), &end, 10);
        if (rank_eval_n.empty() || *end != '\0' || n < 1 || n > 1000) die("--rank-eval expects 1 <= N <= 1000, not '" + rank_eval_n + "'");
        J.rank_eval = (int)n;
        if (rank_by != "rows" && rank_by != "cols") die("--rank-by expects rows or cols, not '" + rank_by + "'");
        J.rank_by_cols = rank_by == "cols";
        if (J.rank_thr_given) {
            J.rank_thr = rank_threshold.empty() ? NAN : strtod(rank_threshold.c_str(), &end);
            if (rank_threshold.empty() || *end != '\0' || !std::isfinite(J.rank_thr)) die("--rank-threshold expects a finite number, not '" + rank_threshold + "'");
        } else if (J.implicit) { J.rank_thr_given = true; J.rank_thr = 0.0; }
        if (ngpu > 1) die("--rank-eval runs on one GPU: -g " + std::to_string(ngpu) + " is not supported (the sharded replicas are not complete on every rank)");
        if (J.nsims <= J.burnin) die("--rank-eval needs at least one post-burn-in sample (-i > -b)");
    }
    // --fold-in-rows / --fold-in-cols: checked before anything touches a GPU (the files themselves below, once the shape is known)
    for (int which = 0; which < 2; ++which) {
        const std::string &name = which ? fold_in_cols : fold_in_rows;
        if (name.empty()) continue;
        const std::string w = which ? "--fold-in-cols" : "--fold-in-rows";
        if (J.odirname.empty()) die(w + " needs -o DIR (the predictions go to files in DIR)");
        if (J.nsims <= J.burnin) die(w + " needs at least one post-burn-in sample (-i > -b)");
        if (ngpu >= 1) die(w + " runs on one GPU without -g: -g " + std::to_string(ngpu) + " is not supported (the sample rings of a sharded side are not complete)");
        if (J.probit) die(w + " does not go together with --probit (labels would need a latent iteration of their own)");
        if (!mname.empty() || !lname.empty()) die(w + " does not go together with a propagated posterior (-m / -l): a new entity has none");
        if (getenv("BPMF_REDUCE") && atoi(getenv("BPMF_REDUCE")) != 0) die(w + " does not go together with BPMF_REDUCE=1");
        if (!(which ? col_features : row_features).empty())
            die(w + " does not go together with " + (which ? "--col-features" : "--row-features") + ": the prior mean of a new " + (which ? "column" : "row") +
                " needs its features (" + (which ? "--new-col-features" : "--new-row-features") + " predicts such " + (which ? "columns" : "rows") + ")");
        if (topn_score != "mean") die(w + " does not go together with --topn-score " + topn_score + " (its lists are ranked by the mean)");
        if (!sparse_file(name)) die(w + ": " + name + " is not a sparse matrix file (.sdm, .sbm or a coordinate .mtx)");
    }
    if (model_given)
        return run_model(J, model_dir, fname, probename, predict_file, predict_threshold_given, predict_thr, fold_in_rows, fold_in_cols, d_given, K);
    // fp64 like the reference (c++/bpmf.h:55-58) for every num_latent; the fp32 large-K path only when asked for
    J.K = K;
    J.dtype = fp32 ? BPMF_HIP_F32 : BPMF_HIP_F64;
    if (!bpmf_hip_supports(K, J.dtype))
        die("unsupported number of latent dimensions " + std::to_string(K) + (fp32 ? " with --fp32 (65 .. 128)" : " (1 .. 128)"));
    if (J.verbose && J.odirname.empty()) die("-v needs -o DIR");   // the reference would write to "/U-0.ddm" 
    // -g N: the sharded path (N = 1 too: one rank with a communicator -- what the tests can run on one GPU); no -g: NO_COMM
    J.sharded = ngpu >= 1;
    J.nranks = std::max(ngpu, 1);

    // Sys::Sys (c++/sample.cpp:112-137): read, grow both to the common shape, transpose for the users
    try {
        J.M = bpmf::io::read_sparse(fname);
        J.T = bpmf::io::read_sparse(probename);
    } catch (const std::exception &e) { die(e.what()); }
    // --censored FILE: the flags as a matrix with the structure of M (value = flag), so that they follow the ratings through the
    // renumbering and the transpose below.  Cells are named in 1-based ids of the input.
    Csc CF;
    if (J.censored) {
        Csc C;
        try { C = bpmf::io::read_sparse(censored_file); } catch (const std::exception &e) { die(e.what()); }
        if (C.nrows != J.M.nrows || C.ncols != J.M.ncols)
            die("--censored: " + censored_file + " is " + std::to_string(C.nrows) + " x " + std::to_string(C.ncols) + ", the training matrix is " +
                std::to_string(J.M.nrows) + " x " + std::to_string(J.M.ncols));
        CF = J.M;
        std::fill(CF.vals.begin(), CF.vals.end(), 0.0);
        for (int64_t c = 0; c < C.ncols; ++c)
            for (int64_t q = C.colptr[(size_t)c]; q < C.colptr[(size_t)c + 1]; ++q) {
                const int32_t r = C.rowidx[(size_t)q];
                const double v = C.vals[(size_t)q];
                const std::string cell = "cell (" + std::to_string((long long)r + 1) + ", " + std::to_string((long long)c + 1) + ")";
                if (!std::isfinite(v) || v == 0.0) die("--censored: the value of " + cell + " of " + censored_file + " is zero or not finite");
                const int32_t *b = J.M.rowidx.data() + J.M.colptr[(size_t)c], *e = J.M.rowidx.data() + J.M.colptr[(size_t)c + 1];
                const int32_t *at = std::lower_bound(b, e, r);
                if (at == e || *at != r) die("--censored: " + cell + " of " + censored_file + " is not a cell of the training matrix");
                CF.vals[(size_t)(at - J.M.rowidx.data())] = v > 0.0 ? 1.0 : -1.0;
                (v > 0.0 ? J.cens_right : J.cens_left) += 1;
            }
    }
    // --weights FILE: the weights as a matrix with the structure of M (1 where FILE lists nothing), so that they follow the ratings
    // through the renumbering and the transpose below.  Cells are named in 1-based ids of the input.
    Csc WF;
    if (J.weighted) {
        Csc W;
        try { W = bpmf::io::read_sparse(weights_file); } catch (const std::exception &e) { die(e.what()); }
        if (W.nrows != J.M.nrows || W.ncols != J.M.ncols)
            die("--weights: " + weights_file + " is " + std::to_string(W.nrows) + " x " + std::to_string(W.ncols) + ", the training matrix is " +
                std::to_string(J.M.nrows) + " x " + std::to_string(J.M.ncols));
        WF = J.M;
        std::fill(WF.vals.begin(), WF.vals.end(), 1.0);
        bool first = true;
        for (int64_t c = 0; c < W.ncols; ++c)
            for (int64_t q = W.colptr[(size_t)c]; q < W.colptr[(size_t)c + 1]; ++q) {
                const int32_t r = W.rowidx[(size_t)q];
                const double v = W.vals[(size_t)q];
                const std::string cell = "cell (" + std::to_string((long long)r + 1) + ", " + std::to_string((long long)c + 1) + ")";
                if (!std::isfinite(v) || !(v > 0.0)) die("--weights: the weight of " + cell + " of " + weights_file + " is not finite and > 0");
                const int32_t *b = J.M.rowidx.data() + J.M.colptr[(size_t)c], *e = J.M.rowidx.data() + J.M.colptr[(size_t)c + 1];
                const int32_t *at = std::lower_bound(b, e, r);
                if (at == e || *at != r) die("--weights: " + cell + " of " + weights_file + " is not a cell of the training matrix");
                WF.vals[(size_t)(at - J.M.rowidx.data())] = v;
                J.w_count += v != 1.0;
                J.w_min = first ? v : std::min(J.w_min, v); J.w_max = first ? v : std::max(J.w_max, v);
                first = false;
            }
        if ((int64_t)W.vals.size() < J.M.nnz()) { J.w_min = std::min(J.w_min, 1.0); J.w_max = std::max(J.w_max, 1.0); }   // (the unlisted cells)
        if (J.implicit)                                              // the weights are the confidences: every one above W0
            for (int64_t c = 0; c < WF.ncols; ++c)
                for (int64_t q = WF.colptr[(size_t)c]; q < WF.colptr[(size_t)c + 1]; ++q)
                    if (!(WF.vals[(size_t)q] > J.implicit_w0)) {
                        char v[32];
                        snprintf(v, sizeof v, "%g", WF.vals[(size_t)q]);
                        die("--implicit " + implicit_w0 + ": the confidence " + v + " of cell (" + std::to_string((long long)WF.rowidx[(size_t)q] + 1) + ", " +
                            std::to_string((long long)c + 1) + ") is not > W0");
                    }
    }
    const int64_t rows = std::max(J.M.nrows, J.T.nrows), cols = std::max(J.M.ncols, J.T.ncols);
    if (J.censored) bpmf::io::resize(CF, rows, cols);
    if (J.weighted) bpmf::io::resize(WF, rows, cols);
    bpmf::io::resize(J.M, rows, cols);
    bpmf::io::resize(J.T, rows, cols);
    if (J.M.nnz() == 0) die("the training matrix is empty");
    J.Mt = bpmf::io::transpose(J.M);
    const int64_t nmovies = cols, nusers = rows;
    double msum = 0.0, usum = 0.0;                              // mean_rating = M.sum()/M.nonZeros() per Sys (:183)
    for (double v : J.M.vals) msum += v;
    for (double v : J.Mt.vals) usum += v;
    J.mean_m = msum / (double)J.M.nnz(); J.mean_u = usum / (double)J.Mt.nnz();
    if (J.probit) J.mean_m = J.mean_u = 0.0;                    // labels, not measurements: the latent scores are centred at 0
    if (J.implicit) J.mean_m = J.mean_u = 0.0;                  // every cell is observed, most of them as zeros: the model has mean 0
    if (J.ordinal) {                                            // levels, not measurements; still before anything touches a GPU
        J.mean_m = J.mean_u = 0.0;
        if (J.ord_levels.empty()) {                             // the distinct training values
            std::vector<double> v(J.M.vals);
            std::sort(v.begin(), v.end());
            v.erase(std::unique(v.begin(), v.end()), v.end());
            if (v.size() < 2 || v.size() > 16)
                die("--ordinal: the training matrix has " + std::to_string(v.size()) + " distinct values (2 .. 16 levels are supported; --ordinal-levels names them)");
            for (double x : v) if (!std::isfinite(x)) die("--ordinal: a training value is not finite");
            J.ord_levels = v;
        }
        if (J.ord_fixed && J.ord_cut0.size() + 1 != J.ord_levels.size())
            die("--ordinal-cutpoints expects " + std::to_string(J.ord_levels.size() - 1) + " cutpoints for " + std::to_string(J.ord_levels.size()) + " levels");
        for (double x : J.M.vals)
            if (!std::binary_search(J.ord_levels.begin(), J.ord_levels.end(), x)) die("--ordinal: the training value " + std::to_string(x) + " is not one of the levels");
        for (double x : J.T.vals)
            if (!std::binary_search(J.ord_levels.begin(), J.ord_levels.end(), x)) die("--ordinal: the test value " + std::to_string(x) + " is not one of the levels");
    }

    auto read_features = [&](const std::string &name, int64_t n, const char *what, Dense &F) {
        if (name.empty()) return;
        try { F = bpmf::io::read_dense(name); } catch (const std::exception &e) { die(e.what()); }
        if (F.nrows != n) die(std::string("--") + what + ": " + name + " has " + std::to_string(F.nrows) + " rows, the side has " + std::to_string(n));
        if (F.ncols < 1 || F.ncols > 1024) die(std::string("--") + what + ": expects 1 .. 1024 feature columns, not " + std::to_string(F.ncols));
    };
    auto read_sparse_features = [&](const std::string &name, int64_t n, const char *what, Csc &Fr, int64_t &D) {
        Csc F;                                                  // N x D, column-compressed
        try { F = bpmf::io::read_sparse(name); } catch (const std::exception &e) { die(e.what()); }
        if (F.nrows != n) die(std::string("--") + what + ": " + name + " has " + std::to_string(F.nrows) + " rows, the side has " + std::to_string(n));
        if (F.ncols < 1 || F.ncols > 0x7FFFFFFF) die(std::string("--") + what + ": expects at least one feature column, not " + std::to_string(F.ncols));
        D = F.ncols;
        Fr = bpmf::io::transpose(F);                            // column i of F^T = row i of F, its feature indices sorted
    };
    if (sparse_u) read_sparse_features(row_features, nusers, "row-features", J.sfeat_u, J.sfeat_u_d);
    else read_features(row_features, nusers, "row-features", J.feat_u);
    if (sparse_m) read_sparse_features(col_features, nmovies, "col-features", J.sfeat_m, J.sfeat_m_d);
    else read_features(col_features, nmovies, "col-features", J.feat_m);

    // the features of the new entities: the same number of feature columns, finite; n x other side within the cap of a dense file
    auto read_new = [&](const std::string &name, bool sparse, int64_t D, int64_t nother, const char *what, const char *partner, Job::NewRows &N) {
        if (name.empty()) return;
        const std::string w = std::string("--") + what;
        // the shape is judged before anything of the file's size is scanned or copied
        auto shape = [&](int64_t n, int64_t d) {
            if (d != D) die(w + ": " + name + " has " + std::to_string(d) + " feature columns, --" + partner + " has " + std::to_string(D));
            if (n < 1) die(w + ": " + name + " has no rows");
            N.n = n;
            if (n > ((int64_t)1 << 28) / std::max<int64_t>(nother, 1)) {
                const std::string cells = std::to_string(n) + " x " + std::to_string(nother) + " predictions are more than 2^28 cells per file";
                if (J.topn < 1) die(w + ": " + cells + ": ask for the best N of every query with --topn N instead");
                std::cerr << w << ": " << cells << ": the dense mean / std files are skipped, the --topn lists are written" << std::endl;
                N.dense_out = false;
            }
        };
        if (sparse) {
            Csc F;
            try { F = bpmf::io::read_sparse(name); } catch (const std::exception &e) { die(e.what()); }
            shape(F.nrows, F.ncols);
            for (double v : F.vals) if (!std::isfinite(v)) die(w + ": " + name + " holds a value that is not finite");
            N.Fr = bpmf::io::transpose(F);
        } else {
            Dense F;
            try { F = bpmf::io::read_dense(name); } catch (const std::exception &e) { die(e.what()); }
            const int64_t n = F.nrows, d = F.ncols;
            shape(n, d);
            for (double v : F.data) if (!std::isfinite(v)) die(w + ": " + name + " holds a value that is not finite");
            N.F.resize((size_t)n * (size_t)d);                          // column-major file -> n x D row-major
            for (int64_t j = 0; j < d; ++j)
                for (int64_t i = 0; i < n; ++i) N.F[(size_t)i * (size_t)d + (size_t)j] = F.data[(size_t)j * (size_t)n + (size_t)i];
        }
    };
    read_new(new_row_features, sparse_u, sparse_u ? J.sfeat_u_d : J.feat_u.ncols, nmovies, "new-row-features", "row-features", J.new_u);
    read_new(new_col_features, sparse_m, sparse_m ? J.sfeat_m_d : J.feat_m.ncols, nusers, "new-col-features", "col-features", J.new_m);

    read_fold(J, fold_in_rows, true, J.fold_u);
    read_fold(J, fold_in_cols, false, J.fold_m);

    // Sys::add_prop_posterior (c++/sample.cpp:157-174): "mu_file,lambda_file"; K x N and K*K x N dense matrices
    auto read_prop = [&](const std::string &fnames, int64_t n, const char *what, Dense &mu, Dense &lambda) {
        if (fnames.empty()) return;
        const size_t pos = fnames.find_first_of(",");
        if (pos == std::string::npos) die(std::string("-") + what + " expects MU_FILE,LAMBDA_FILE");
        try {
            mu = bpmf::io::read_dense(fnames.substr(0, pos));
            lambda = bpmf::io::read_dense(fnames.substr(pos + 1));
        } catch (const std::exception &e) { die(e.what()); }
        if (mu.ncols != n || lambda.ncols != n || mu.nrows != K || lambda.nrows != (int64_t)K * K)
            die(std::string("propagated posterior (-") + what + "): expected " + std::to_string(K) + " x " + std::to_string(n) + " and " +
                std::to_string(K * K) + " x " + std::to_string(n) + " matrices");
    };
    read_prop(mname, nmovies, "m", J.prop_m_mu, J.prop_m_lambda);
    read_prop(lname, nusers, "l", J.prop_u_mu, J.prop_u_lambda);

    // Assignment of the columns to the GPUs.  -k: equal column counts (c++/assign.cpp:60-65).  Otherwise the reference's
    // greedy, permuting assign() (BPMF_ASSIGN=greedy, the default with more than one GPU: `bpmf -g N` then behaves like
    // `mpirun -np N bpmf`, including column ids -- and RNG streams -- that depend on N), or BPMF_ASSIGN=contiguous:
    // cuts of the original order at equal work, which keep the samples independent of N.
    const char *assign_env = getenv("BPMF_ASSIGN");
    // (test hook: BPMF_TEST_ASSIGN_PARTS=P renumbers as for P ranks while running on the ranks there are -- what one
    // GPU can check of the permute / unpermute plumbing)
    const int assign_parts = getenv("BPMF_TEST_ASSIGN_PARTS") ? atoi(getenv("BPMF_TEST_ASSIGN_PARTS")) : J.nranks;
    const bool greedy = balance && assign_parts > 1 && !(assign_env && std::string(assign_env) == "contiguous");
    if (greedy && (J.fold_u.n > 0 || J.fold_m.n > 0)) die("--fold-in-rows / --fold-in-cols do not go together with a renumbering assignment of the columns");
    if (greedy && linked) die("--row-features / --col-features do not go together with a renumbering assignment of the columns");
    if (greedy) {
        J.perm_m.resize((size_t)nmovies); J.perm_u.resize((size_t)nusers);
        for (int64_t i = 0; i < nmovies; ++i) J.perm_m[(size_t)i] = i;
        for (int64_t i = 0; i < nusers; ++i) J.perm_u[(size_t)i] = i;
        std::vector<int64_t> dm((size_t)assign_parts + 1, 0), du((size_t)assign_parts + 1, 0);
        for (int pass = 0; pass < 2; ++pass) {                       // movies.assign(users); users.assign(movies); twice (c++/bpmf.cpp:140-143)
            for (int side = 0; side < 2; ++side) {
                std::vector<int64_t> &perm = side == 0 ? J.perm_m : J.perm_u;
                const Csc &A = side == 0 ? J.M : J.Mt;
                std::vector<int64_t> cp(perm.size() + 1, 0), order(perm.size());
                for (size_t j = 0; j < perm.size(); ++j) cp[j + 1] = cp[j] + (A.colptr[(size_t)perm[j] + 1] - A.colptr[(size_t)perm[j]]);
                if (bpmf_assign_greedy((int64_t)perm.size(), cp.data(), assign_parts, order.data(), side == 0 ? dm.data() : du.data()))
                    die("assignment failed");
                std::vector<int64_t> np(perm.size());
                for (size_t j = 0; j < perm.size(); ++j) np[j] = perm[(size_t)order[j]];
                perm.swap(np);
            }
        }
        if (assign_parts == J.nranks) { J.bm = dm; J.bu = du; }
        else { J.bm = {0, nmovies}; J.bu = {0, nusers}; if (J.nranks != 1) die("BPMF_TEST_ASSIGN_PARTS needs one rank"); }
        const std::vector<int64_t> inv_u = inverse(J.perm_u);
        J.M = permute(J.M, J.perm_m, inv_u);
        J.T = permute(J.T, J.perm_m, inv_u);
        if (J.censored) CF = permute(CF, J.perm_m, inv_u);
        if (J.weighted) WF = permute(WF, J.perm_m, inv_u);
        J.Mt = bpmf::io::transpose(J.M);
        permute_columns(J.prop_m_mu.data, K, J.perm_m); permute_columns(J.prop_m_lambda.data, (int64_t)K * K, J.perm_m);
        permute_columns(J.prop_u_mu.data, K, J.perm_u); permute_columns(J.prop_u_lambda.data, (int64_t)K * K, J.perm_u);
    } else {
        J.bm = column_ranges(J.M, J.nranks, balance);
        J.bu = column_ranges(J.Mt, J.nranks, balance);
    }
    // BPMF_HIP_DEVICES=d0,d1,...: the HIP device of every rank (default: rank r on device r).  Two ranks on one device
    // need a communication library that serves them (BPMF_HIP_RCCL_LIBRARY: RCCL itself refuses) -- the tests' set-up.
    if (const char *e = getenv("BPMF_HIP_DEVICES")) {
        std::stringstream ss(e);
        std::string tok;
        while (std::getline(ss, tok, ',')) if (!tok.empty()) J.devices.push_back(atoi(tok.c_str()));
    }
    if (J.censored) {                                                // (CF has the structure of M, its transpose that of Mt)
        const Csc CFt = bpmf::io::transpose(CF);
        J.cens_m.assign(std::max<size_t>(CF.vals.size(), 1), 0); J.cens_u.assign(std::max<size_t>(CFt.vals.size(), 1), 0);
        for (size_t q = 0; q < CF.vals.size(); ++q) J.cens_m[q] = (int8_t)CF.vals[q];
        for (size_t q = 0; q < CFt.vals.size(); ++q) J.cens_u[q] = (int8_t)CFt.vals[q];
    }
    if (J.weighted) {                                                // (WF has the structure of M, its transpose that of Mt)
        const Csc WFt = bpmf::io::transpose(WF);
        J.w_m = WF.vals; J.w_u = WFt.vals;
        if (J.w_m.empty()) { J.w_m.assign(1, 1.0); J.w_u.assign(1, 1.0); }
    }
    J.Tt = bpmf::io::transpose(J.T);
    build_rank_lists(J);
    if (J.sharded) check(bpmf_hip_comm_unique_id(J.rccl_id));      // (also loads RCCL before the rank threads start)
    if (!J.odirname.empty()) {
        J.pavg.assign(J.T.vals.size(), 0.0); J.pm2.assign(J.T.vals.size(), 0.0);
        const double nan = std::nan("");                              // (no post-burn-in sample: the reference divides 0 by 0)
        J.u_mu.assign((size_t)K * nusers, nan); J.u_lambda.assign((size_t)K * K * nusers, nan);
        J.m_mu.assign((size_t)K * nmovies, nan); J.m_lambda.assign((size_t)K * K * nmovies, nan);
        // (bpmf_hip_side_aggr_finalize: a covariance of n samples has rank n - 1 at most)
        if (J.nsims - J.burnin <= K)
            std::cerr << "note: U-Lambda.ddm / V-Lambda.ddm are NaN: the " << std::max(J.nsims - J.burnin, 0) << " kept samples (-i " << J.nsims
                      << " -b " << J.burnin << ") do not determine a " << K << " x " << K << " covariance; keep more than " << K << std::endl;
    }

    // stdout of the ranks: bpmf_<rank>.out when there are several or with -r (c++/bpmf.cpp:111-117)
    const bool to_files = J.nranks > 1 || J.redirect;
    std::vector<std::unique_ptr<std::ofstream>> files;
    auto rank_os = [&](int r) -> std::ostream & {
        if (!to_files) return std::cout;
        return *files[(size_t)r];
    };
    if (to_files) for (int r = 0; r < J.nranks; ++r) {
        // emptied, then opened in APPEND mode: die() adds its line through a descriptor of its own (O_APPEND), and a rank thread
        // that writes its next line afterwards must append behind it, not overwrite it at its own file offset
        const std::string name = "bpmf_" + std::to_string(r) + ".out";
        { std::ofstream empty(name, std::ios::out | std::ios::trunc); }
        files.emplace_back(new std::ofstream(name, std::ios::out | std::ios::app));
        g_rank_files.push_back(name);
    }

    if (J.nranks == 1) {
        rank_main(J, 0, rank_os(0));
    } else {
        std::vector<std::thread> th;
        g_rank_threads.store(true);
        for (int r = 0; r < J.nranks; ++r) th.emplace_back([&J, r, &rank_os] { rank_main(J, r, rank_os(r)); });
        for (auto &t : th) t.join();
        g_rank_threads.store(false);
    }
    std::ostream &os = rank_os(0);

    if (!J.odirname.empty()) {
        try {
            // everything that is written is in the ORIGINAL numbering (users.unpermuteCols / movies.unpermuteCols,
            // c++/bpmf.cpp:223-224; the reference leaves items() / aggrMu in the permuted order: not reproduced)
            Csc P = J.T;
            P.vals = J.pavg;
            if (!J.perm_m.empty()) P = permute(P, inverse(J.perm_m), J.perm_u);
            bpmf::io::write_sparse(J.odirname + "/Pavg.sdm", P);
            P = J.T; P.vals = J.pm2;
            if (!J.perm_m.empty()) P = permute(P, inverse(J.perm_m), J.perm_u);
            bpmf::io::write_sparse(J.odirname + "/Pm2.sdm", P);
            if (J.robust && J.robust_w.size() == J.M.vals.size() && !J.robust_w.empty()) {    // (no kept sample: no file)
                P = J.M; P.vals = J.robust_w;
                if (!J.perm_m.empty()) P = permute(P, inverse(J.perm_m), J.perm_u);
                bpmf::io::write_sparse(J.odirname + "/robust-weights.sdm", P);
            }
            if (J.bias) {
                // row-bias.ddm / col-bias.ddm: the posterior-mean bias of every user / movie (1 x n; no kept sample: no file);
                // bias_lambda.csv: the precision either side's step ran with, per iteration
                if (!J.perm_m.empty()) { permute_columns(J.bias_u, 1, inverse(J.perm_u)); permute_columns(J.bias_m, 1, inverse(J.perm_m)); }
                Dense b;
                if (!J.bias_u.empty()) { b.nrows = 1; b.ncols = nusers; b.data = J.bias_u; bpmf::io::write_dense(J.odirname + "/row-bias.ddm", b); }
                if (!J.bias_m.empty()) { b.nrows = 1; b.ncols = nmovies; b.data = J.bias_m; bpmf::io::write_dense(J.odirname + "/col-bias.ddm", b); }
                std::ofstream csv(J.odirname + "/bias_lambda.csv");
                csv << "iteration,lambda_rows,lambda_cols\n";
                csv.precision(17);
                for (size_t i = 0; i < J.bias_lam_u.size(); ++i) csv << i << "," << J.bias_lam_u[i] << "," << J.bias_lam_m[i] << "\n";
                if (!csv) throw std::runtime_error("cannot write " + J.odirname + "/bias_lambda.csv");
            }
            if (!J.perm_m.empty()) {
                const std::vector<int64_t> im = inverse(J.perm_m), iu = inverse(J.perm_u);
                permute_columns(J.u_mu, K, iu); permute_columns(J.u_lambda, (int64_t)K * K, iu);
                permute_columns(J.m_mu, K, im); permute_columns(J.m_lambda, (int64_t)K * K, im);
            }
            Dense d;
            d.nrows = K; d.ncols = nusers; d.data.swap(J.u_mu);
            bpmf::io::write_dense(J.odirname + "/U-mu.ddm", d);
            d.nrows = (int64_t)K * K; d.data.swap(J.u_lambda);
            bpmf::io::write_dense(J.odirname + "/U-Lambda.ddm", d);
            d.nrows = K; d.ncols = nmovies; d.data.swap(J.m_mu);
            bpmf::io::write_dense(J.odirname + "/V-mu.ddm", d);
            d.nrows = (int64_t)K * K; d.data.swap(J.m_lambda);
            bpmf::io::write_dense(J.odirname + "/V-Lambda.ddm", d);
            auto write_link = [&](const std::vector<double> &beta, const char *name) {     // D x K, row-major -> column-major
                if (beta.empty()) return;
                Dense b;
                b.nrows = (int64_t)(beta.size() / (size_t)K); b.ncols = K; b.data.resize(beta.size());
                for (int64_t dd = 0; dd < b.nrows; ++dd)
                    for (int k = 0; k < K; ++k) b.data[(size_t)k * (size_t)b.nrows + (size_t)dd] = beta[(size_t)dd * K + k];
                bpmf::io::write_dense(J.odirname + name, b);
            };
            write_link(J.beta_u, "/U-link.ddm");
            write_link(J.beta_m, "/V-link.ddm");
        } catch (const std::exception &e) { die(e.what()); }
    }

    write_topn(J);
    write_similar(J);
    write_diag(J);
    write_score(J, &J.T, &J.M);
    write_intervals(J);
    write_loo(J, J.M);

    const RankMetrics rkm = write_ranks(J);

    write_new(J, J.new_u, true, nmovies, "new");
    write_new(J, J.new_m, false, nusers, "new");

    // the folded-in entities: the same layout, queries numbered by their row (column) in FILE
    write_new(J, J.fold_u, true, nmovies, "foldin");
    write_new(J, J.fold_m, false, nusers, "foldin");

    if (J.lb_sampled && !J.odirname.empty()) {                       // a cell is empty where a side has no features
        FILE *f = fopen((J.odirname + "/lambda_beta.csv").c_str(), "w");
        if (!f) die("cannot write " + J.odirname + "/lambda_beta.csv");
        fprintf(f, "iteration,lambda_rows,lambda_cols\n");
        const size_t n = std::max(J.lb_trace_u.size(), J.lb_trace_m.size());
        for (size_t i = 0; i < n; ++i) {
            fprintf(f, "%zu,", i);
            if (i < J.lb_trace_u.size()) fprintf(f, "%.17g", J.lb_trace_u[i]);
            fprintf(f, ",");
            if (i < J.lb_trace_m.size()) fprintf(f, "%.17g", J.lb_trace_m[i]);
            fprintf(f, "\n");
        }
        if (fclose(f) != 0) die("cannot write " + J.odirname + "/lambda_beta.csv");
    }

    if (J.adaptive && !J.odirname.empty()) {
        FILE *f = fopen((J.odirname + "/alpha.csv").c_str(), "w");
        if (!f) die("cannot write " + J.odirname + "/alpha.csv");
        fprintf(f, "iteration,alpha,train_rmse\n");
        for (size_t i = 0; i < J.alpha_trace.size(); ++i) fprintf(f, "%zu,%.17g,%.17g\n", i, J.alpha_trace[i], J.train_rmse[i]);
        if (fclose(f) != 0) die("cannot write " + J.odirname + "/alpha.csv");
    }

    if (J.probit && !J.odirname.empty() && !J.prob.empty()) {        // test-set order of T, 1-based ids in the ORIGINAL numbering
        FILE *f = fopen((J.odirname + "/probit.csv").c_str(), "w");
        if (!f) die("cannot write " + J.odirname + "/probit.csv");
        fprintf(f, "row,col,label,prob\n");
        for (int64_t c = 0; c < J.T.ncols; ++c)
            for (int64_t q = J.T.colptr[(size_t)c]; q < J.T.colptr[(size_t)c + 1]; ++q) {
                const int64_t r = J.T.rowidx[(size_t)q];
                fprintf(f, "%lld,%lld,%d,%.17g\n", (long long)((J.perm_u.empty() ? r : J.perm_u[(size_t)r]) + 1),
                        (long long)((J.perm_m.empty() ? c : J.perm_m[(size_t)c]) + 1), J.T.vals[(size_t)q] > J.probit_threshold ? 1 : 0,
                        J.prob[(size_t)q]);
            }
        if (fclose(f) != 0) die("cannot write " + J.odirname + "/probit.csv");
    }

    if (J.ordinal && !J.odirname.empty()) {
        const size_t C = J.ord_levels.size();
        if (!J.cat_prob.empty()) {                                   // test-set order of T, 1-based ids in the ORIGINAL numbering
            FILE *f = fopen((J.odirname + "/ordinal.csv").c_str(), "w");
            if (!f) die("cannot write " + J.odirname + "/ordinal.csv");
            fprintf(f, "row,col,value,expected");
            for (size_t k = 0; k < C; ++k) fprintf(f, ",p%zu", k + 1);
            fprintf(f, "\n");
            for (int64_t c = 0; c < J.T.ncols; ++c)
                for (int64_t q = J.T.colptr[(size_t)c]; q < J.T.colptr[(size_t)c + 1]; ++q) {
                    const int64_t r = J.T.rowidx[(size_t)q];
                    const double *p = &J.cat_prob[(size_t)q * C];
                    double e = 0.0;
                    for (size_t k = 0; k < C; ++k) e += J.ord_levels[k] * p[k];
                    fprintf(f, "%lld,%lld,%.17g,%.17g", (long long)((J.perm_u.empty() ? r : J.perm_u[(size_t)r]) + 1),
                            (long long)((J.perm_m.empty() ? c : J.perm_m[(size_t)c]) + 1), J.T.vals[(size_t)q], e);
                    for (size_t k = 0; k < C; ++k) fprintf(f, ",%.17g", p[k]);
                    fprintf(f, "\n");
                }
            if (fclose(f) != 0) die("cannot write " + J.odirname + "/ordinal.csv");
        }
        FILE *f = fopen((J.odirname + "/cutpoints.csv").c_str(), "w");
        if (!f) die("cannot write " + J.odirname + "/cutpoints.csv");
        fprintf(f, "iteration,accepted,step");
        for (size_t k = 1; k < C; ++k) fprintf(f, ",g%zu", k);
        fprintf(f, "\n");
        for (size_t i = 0; i < J.ord_accepted.size(); ++i) {
            fprintf(f, "%zu,%d,%.17g", i, J.ord_accepted[i], J.ord_step_trace[i]);
            for (size_t k = 0; k + 1 < C; ++k) fprintf(f, ",%.17g", J.ord_trace[i * (C - 1) + k]);
            fprintf(f, "\n");
        }
        if (fclose(f) != 0) die("cannot write " + J.odirname + "/cutpoints.csv");
    }

    os << "Total time: " << J.elapsed << std::endl;
    os << "Final Avg RMSE: " << J.rmse_avg << std::endl;
    print_diag(os, J, true);
    print_score(os, J);
    print_intervals(os, J);
    print_loo(os, J);
    if (J.ordinal && !J.cat_prob.empty()) {
        os << "Final ordinal RMSE: " << J.ord_rmse << std::endl;
        os << "Final accuracy: " << J.ord_accuracy << std::endl;
        os << "Final log-prob: " << J.ord_logp << std::endl;
    }
    if (J.probit && !J.prob.empty()) {
        os << "Final AUC: " << J.auc << std::endl;
        os << "Final Brier: " << J.brier << std::endl;
    }
    if (J.rank_eval > 0) {
        os << "Final recall@" << J.rank_eval << ": " << rkm.recall << std::endl;
        os << "Final NDCG@" << J.rank_eval << ": " << rkm.ndcg << std::endl;
        os << "Final MRR: " << rkm.mrr << std::endl;
        os << "Final MPR: " << rkm.mpr << std::endl;
        os << "Final rank AUC: " << rkm.auc << std::endl;
    }
    os << "  computed on " << J.num_predict << " items (" << (J.T.nnz() ? int(100. * (double)J.num_predict / (double)J.T.nnz()) : 0)
       << "% of total items in test set)" << std::endl;
    // the reference divides by movies.iter = nsims-1; this build reports the true mean
    os << "Average items/sec: " << (double)(J.average_items_sec / std::max(J.nsims, 1)) << std::endl;
    os << "Average ratings/sec: " << (double)(J.average_ratings_sec / std::max(J.nsims, 1)) << std::endl;
    return 0;
}

{-# LANGUAGE ForeignFunctionInterface #-}
{-# LANGUAGE ScopedTypeVariables #-}

-- |
-- Module      :  McmcDate.GpuSampler
-- Description :  Reference-side binding of the FAST path: the lock-step Metropolis-Hastings driver on an MI355X
--
-- SOURCE ONLY (no GHC / cabal / stack in the build image; see "McmcDate.Gpu" for the literal drop-in of the likelihood closure).
--
-- The literal drop-in -- one state per call through 'McmcDate.Gpu.likelihoodFunctionGpu' -- costs a launch and a round trip per
-- proposal (15 - 25 us, INTEGRATION.md): slower than the CPU closure at the reference's sizes.  The speed of the library lives in
-- @mcd_mh_run@: B chains stepping together on the device through the reference's whole proposal cycle, nothing crossing the bus
-- between monitor periods.  This module is the replacement of @runMetropolisHastingsGreen@ (app/Main.hs:460-479) that uses it:
--
--   * 'proposalTable' builds the table @mcd_mh_create@ takes from the SAME definitions as 'Definitions.proposals'
--     (app/Definitions.hs:127-278): order, names, weights, standard deviations / shapes, 'PDimension's, which proposals are lifted
--     with 'jacobianRootBranch' ("[R]"), node paths as pre-order ids ('identify', the numbering of the calibrations);
--   * 'runMetropolisHastingsGreenGpu' runs the burn-in schedule with auto tuning ('Definitions.burnIn', :420-424) and the iterations
--     (:440-441) in blocks of the monitor period (2, :288-417): @mcd_mh_run@ per block, @mcd_mh_tune@ per tuning period,
--     @mcd_mh_get_state@ per block -> the chains' states as values of 'I', handed to the caller's monitor action (the reference's
--     'Definitions.monitor' executes on an 'I'); @mcd_mh_get_age_sums@ at the end for the node-age summary of @scripts/analyze@;
--   * 'runRecorded' is the same loop without the cut at every monitor period: the device keeps the samples while a chunk of
--     iterations runs in ONE @mcd_mh_run@ (@mcd_mh_record_begin@ / @_fetch@ / @_end@), and the monitor action is called from the
--     fetched samples, one @mcd_mh_record_fetch@ per chunk instead of one @mcd_mh_get_state@ per two iterations;
--   * 'recordSummary' asks the device for the node-age summary, split R-hat and effective sample size of the samples the recorder
--     holds (@mcd_mh_record_summary@) instead of fetching them;
--   * 'withHamiltonian' is @--hamiltonian@ ('maybeHamiltonianProposal', app/Definitions.hs:272-278): for the duration of an action a
--     leapfrog handle is attached to the driver (@mcd_mh_attach_hamiltonian@) and every iteration of the loops above begins with one NUTS
--     transition of every chain, the chains moving between the two drivers on the device;
--   * 'runMc3Gpu' is @mc3 (MC3Settings (NChains 4) (SwapPeriod 2) (NSwaps 3))@ (app/Main.hs:476-478): @mcd_mh_mc3_init@, per swap
--     period @mcd_mh_run@ + @mcd_mh_mc3_swap@, the monitors read the chains whose temperature rank is 0 (@mcd_mh_mc3_get@).
--
-- The likelihood is whichever handle 'getLikelihoodHandle' made from the @.data@ record: the dense factor (@Full@, @Univariate@) or
-- the precision matrix kept sparse on the device (@Sparse@: the production configuration, app/Main.hs:257-277 -> @mcd_mh_create_sparse@).
--
-- INTEGRATION.md, "fourth edit", shows the six lines of app/Main.hs that change.
module McmcDate.GpuSampler
  ( ProposalRow (..),
    proposalTable,
    cycleSchedule,
    LikelihoodHandle (..),
    GpuSampler,
    withGpuSampler,
    runMetropolisHastingsGreenGpu,
    -- checkpoint and continue (@Settings ... Save@, @continue@, @--init-from-save@)
    CheckpointMode (..),
    saveSampler,
    loadSampler,
    continueMetropolisHastingsGreenGpu,
    runMarginalLikelihoodGpu,
    runRecorded,
    recordSummary,
    runMc3Gpu,
    nodeAgeSummary,
    -- the Hamiltonian proposal in the cycle (@--hamiltonian@)
    withHamiltonian,
    setHamiltonianTransitionForm,
    c_hmc_take_state,
    c_mh_take_state,
    -- the NUTS driver's recorder, raw (the handle comes from 'McmcDate.Gpu')
    c_hmc_record_begin,
    c_hmc_record_count,
    c_hmc_record_fetch,
    c_hmc_record_end,
    c_hmc_record_quantities,
    c_hmc_record_summary,
    -- the form of the NUTS driver's dense metric, raw
    c_hmc_set_metric_form,
    c_hmc_get_metric_form,
    -- where the dense metric's factors are taken, raw
    c_hmc_set_metric_factor,
    c_hmc_get_metric_factor,
    -- how the NUTS driver launches a transition, raw
    c_hmc_set_transition_form,
    c_hmc_get_transition_form,
  )
where

import Control.Lens ((&), (.~), (^.))
import Control.Monad (forM_, replicateM, when)
import Data.Int (Int32, Int64, Int8)
import Data.List (foldl')
import qualified Data.Vector.Storable as VS
import qualified Data.Vector.Storable.Mutable as VSM
import Data.Word (Word64)
import qualified ELynx.Tree as T
import Foreign
import Foreign.C.String
import Foreign.C.Types
import Mcmc.Tree (HeightTree (..), LengthTree (..), getHeightTree, getLengthTree)
import McmcDate.Gpu (McdHmc, McdMh, McdPrior, McdSparseTree, McdTree)
import State (I, IG (..), rateMean, rateTree, rateVariance, timeBirthRate, timeDeathRate, timeHeight, timeTree)
import System.Random.Stateful (StatefulGen, uniformRM)

-- ---------------------------------------------------------------------------------------------------------------------------------
-- include/mcmcdate_mvn.h: the entry points the loop needs, with the header's signatures (tests/test_host.py checks names and
-- arities of every import of this module against the library's symbol table)
-- ---------------------------------------------------------------------------------------------------------------------------------
foreign import ccall unsafe "mcd_last_error"
  c_last_error :: IO CString

foreign import ccall unsafe "mcd_mh_create"
  c_mh_create ::
    Ptr (Ptr McdMh) -> Ptr McdTree -> Ptr McdPrior -> CInt -> Ptr Int32 -> Ptr Int32 -> Ptr Int32 -> Ptr Int32 -> Ptr Int32 -> Ptr Int32 ->
    Ptr CDouble -> Ptr CDouble -> Int64 -> Word64 -> IO CInt

foreign import ccall unsafe "mcd_mh_create_sparse"
  c_mh_create_sparse ::
    Ptr (Ptr McdMh) -> Ptr McdSparseTree -> Ptr McdPrior -> CInt -> Ptr Int32 -> Ptr Int32 -> Ptr Int32 -> Ptr Int32 -> Ptr Int32 -> Ptr Int32 ->
    Ptr CDouble -> Ptr CDouble -> Int64 -> Word64 -> IO CInt

foreign import ccall unsafe "mcd_mh_destroy"
  c_mh_destroy :: Ptr McdMh -> IO ()

foreign import ccall unsafe "mcd_mh_set_chain_offset"
  c_mh_set_chain_offset :: Ptr McdMh -> Int64 -> IO CInt

foreign import ccall unsafe "mcd_mh_set_state"
  c_mh_set_state ::
    Ptr McdMh -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> IO CInt

foreign import ccall unsafe "mcd_mh_get_state"
  c_mh_get_state ::
    Ptr McdMh -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> IO CInt

foreign import ccall unsafe "mcd_mh_get_posterior"
  c_mh_get_posterior :: Ptr McdMh -> Ptr CDouble -> IO CInt

-- (safe: a block of iterations runs for milliseconds to seconds; other Haskell threads go on)
foreign import ccall safe "mcd_mh_run"
  c_mh_run :: Ptr McdMh -> Ptr Int32 -> Int64 -> Int32 -> CInt -> Ptr CDouble -> Ptr Int8 -> IO CInt

foreign import ccall unsafe "mcd_mh_tune"
  c_mh_tune :: Ptr McdMh -> IO CInt

foreign import ccall unsafe "mcd_mh_get_tuning"
  c_mh_get_tuning :: Ptr McdMh -> Ptr CDouble -> Ptr Int32 -> Ptr Int32 -> IO CInt

foreign import ccall unsafe "mcd_mh_reset_counters"
  c_mh_reset_counters :: Ptr McdMh -> IO CInt

foreign import ccall unsafe "mcd_mh_get_age_sums"
  c_mh_get_age_sums :: Ptr McdMh -> Ptr CDouble -> Ptr CDouble -> Ptr Int64 -> IO CInt

foreign import ccall unsafe "mcd_mh_reset_age_sums"
  c_mh_reset_age_sums :: Ptr McdMh -> IO CInt

foreign import ccall unsafe "mcd_mh_set_power"
  c_mh_set_power :: Ptr McdMh -> Ptr CDouble -> IO CInt

foreign import ccall safe "mcd_mh_record_marginal"
  c_mh_record_marginal :: Ptr McdMh -> CInt -> Ptr CDouble -> Int64 -> Int64 -> Ptr Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt

foreign import ccall unsafe "mcd_mh_last_path"
  c_mh_last_path :: Ptr McdMh -> IO CInt

foreign import ccall unsafe "mcd_mh_mc3_init"
  c_mh_mc3_init :: Ptr McdMh -> CInt -> Ptr CDouble -> Int64 -> Word64 -> IO CInt

foreign import ccall unsafe "mcd_mh_mc3_swap"
  c_mh_mc3_swap :: Ptr McdMh -> CInt -> Ptr CDouble -> CInt -> Int64 -> IO CInt

foreign import ccall unsafe "mcd_mh_mc3_get"
  c_mh_mc3_get :: Ptr McdMh -> Ptr Int32 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> IO CInt

-- the sample recorder: thinned samples kept on the device while mcd_mh_run runs (what 'runRecorded' drains)
foreign import ccall unsafe "mcd_mh_record_begin"
  c_mh_record_begin :: Ptr McdMh -> Int32 -> Int64 -> IO CInt

foreign import ccall unsafe "mcd_mh_record_count"
  c_mh_record_count :: Ptr McdMh -> Ptr Int64 -> IO CInt

foreign import ccall unsafe "mcd_mh_record_fetch"
  c_mh_record_fetch ::
    Ptr McdMh -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt

foreign import ccall unsafe "mcd_mh_record_end"
  c_mh_record_end :: Ptr McdMh -> IO CInt

foreign import ccall unsafe "mcd_mh_record_quantities"
  c_mh_record_quantities :: Ptr McdMh -> Ptr Int64 -> IO CInt

-- (safe: several passes over the whole ring)
foreign import ccall safe "mcd_mh_record_summary"
  c_mh_record_summary :: Ptr McdMh -> Int64 -> Int64 -> Int32 -> Ptr Int64 -> Ptr CDouble -> Ptr CDouble -> IO CInt

-- the same recorder on the NUTS driver (runs with @--hamiltonian@; the handle is 'McmcDate.Gpu.McdHmc'): every transition through
-- @mcd_hmc_nuts@ / @_nuts_run@ / @_nuts_warmup@ counts, a sample carries the transition's diagnostics (depth, leapfrog steps, acceptance
-- statistic, diverged, step size, -H at the start) where a Metropolis-Hastings sample carries its temperature
foreign import ccall unsafe "mcd_hmc_record_begin"
  c_hmc_record_begin :: Ptr McdHmc -> Int32 -> Int64 -> IO CInt

foreign import ccall unsafe "mcd_hmc_record_count"
  c_hmc_record_count :: Ptr McdHmc -> Ptr Int64 -> IO CInt

foreign import ccall unsafe "mcd_hmc_record_fetch"
  c_hmc_record_fetch ::
    Ptr McdHmc -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt

foreign import ccall unsafe "mcd_hmc_record_end"
  c_hmc_record_end :: Ptr McdHmc -> IO CInt

foreign import ccall unsafe "mcd_hmc_record_quantities"
  c_hmc_record_quantities :: Ptr McdHmc -> Ptr Int64 -> IO CInt

-- (safe: several passes over the whole ring)
foreign import ccall safe "mcd_hmc_record_summary"
  c_hmc_record_summary :: Ptr McdHmc -> Int64 -> Int64 -> Int32 -> Ptr Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt

-- the form of the dense metric's products (@HTuneAllMasses@ beyond 512 coordinates): 0 = one workgroup's sum per chain (the default),
-- 1 = one matrix product across the lock-step chains, every dim; to be chosen before @mcd_hmc_set_metric@ / @mcd_hmc_nuts_warmup_dense@
foreign import ccall unsafe "mcd_hmc_set_metric_form"
  c_hmc_set_metric_form :: Ptr McdHmc -> CInt -> IO CInt

foreign import ccall unsafe "mcd_hmc_get_metric_form"
  c_hmc_get_metric_form :: Ptr McdHmc -> Ptr CInt -> IO CInt

-- where the factors of the dense metric are taken: 0 = on the host (the default), 1 = on the device (@csrc/k_metric_factor.hip@; the
-- window covariance of @mcd_hmc_nuts_warmup_dense@ then never leaves the GPU); allowed at any time, decides the next factorisation
foreign import ccall unsafe "mcd_hmc_set_metric_factor"
  c_hmc_set_metric_factor :: Ptr McdHmc -> CInt -> IO CInt

foreign import ccall unsafe "mcd_hmc_get_metric_factor"
  c_hmc_get_metric_factor :: Ptr McdHmc -> Ptr CInt -> IO CInt

-- how a transition is launched: 0 = rounds of three launches with a host poll each (the default), 1 = the whole transition as one launch
-- (@csrc/k_nuts_chain.hip@: dense likelihoods of up to 64 distances, i.e. trees of up to 66 nodes; the same bits); allowed at any time
foreign import ccall unsafe "mcd_hmc_set_transition_form"
  c_hmc_set_transition_form :: Ptr McdHmc -> CInt -> IO CInt

foreign import ccall unsafe "mcd_hmc_get_transition_form"
  c_hmc_get_transition_form :: Ptr McdHmc -> Ptr CInt -> IO CInt

-- the Hamiltonian proposal in the cycle (@--hamiltonian@: 'maybeHamiltonianProposal', app/Definitions.hs:272-278): the chains move between
-- the two drivers on the device, and an attached @mcd_hmc_t@ makes one NUTS transition in front of every iteration of @mcd_mh_run@
foreign import ccall unsafe "mcd_hmc_take_state"
  c_hmc_take_state :: Ptr McdHmc -> Ptr McdMh -> IO CInt

foreign import ccall unsafe "mcd_mh_take_state"
  c_mh_take_state :: Ptr McdMh -> Ptr McdHmc -> IO CInt

foreign import ccall unsafe "mcd_mh_attach_hamiltonian"
  c_mh_attach_hamiltonian :: Ptr McdMh -> Ptr McdHmc -> Ptr CDouble -> Ptr CDouble -> CInt -> Word64 -> Word64 -> IO CInt

foreign import ccall unsafe "mcd_mh_detach_hamiltonian"
  c_mh_detach_hamiltonian :: Ptr McdMh -> IO CInt

foreign import ccall unsafe "mcd_mh_hamiltonian_stats"
  c_mh_hamiltonian_stats :: Ptr McdMh -> Ptr Int64 -> Ptr CDouble -> Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> CInt -> IO CInt

-- checkpoint and continue (@Settings ... Save@ and @continue@, app/Main.hs:494-509; @--init-from-save@, :424-440): the handle between two
-- runs as one blob
foreign import ccall unsafe "mcd_mh_save_size"
  c_mh_save_size :: Ptr McdMh -> Ptr Int64 -> IO CInt

foreign import ccall safe "mcd_mh_save"
  c_mh_save :: Ptr McdMh -> Ptr Word8 -> Int64 -> Ptr Int64 -> IO CInt

foreign import ccall safe "mcd_mh_load"
  c_mh_load :: Ptr McdMh -> Ptr Word8 -> Int64 -> CInt -> IO CInt

check :: String -> CInt -> IO ()
check _ 0 = pure ()
check ctx _ = c_last_error >>= peekCString >>= \m -> error (ctx <> ": " <> m)

-- ---------------------------------------------------------------------------------------------------------------------------------
-- The proposal table (MCD_PROP_* of the header; the Python mirror of the same table is mcmc-date_amd/sampler.py: proposals)
-- ---------------------------------------------------------------------------------------------------------------------------------
data ProposalRow = ProposalRow
  { prName :: String,
    prKind :: Int32,
    prNode :: Int32,
    prN1 :: Int32,
    prN2 :: Int32,
    prJacRoot :: Int32, -- liftProposalWith jacobianRootBranch: the "[R]" proposals
    prDim :: Int32, -- PDimension
    prP0 :: Double, -- standard deviation or gamma shape
    prP1 :: Double,
    prWeight :: Int -- PWeight
  }

kScaleScalar, kSlideNode, kScaleSubTreeTime, kPulley, kScaleBranchRate, kScaleSubTreeRate, kScaleNormTree, kScaleVarTree, kScaleVarTreeAuto, kScaleContrarily, kSlideNodeContra, kScaleSubTreeContra, kSlideRootContra, kScaleRatesTreeContra, kSlideBrace, kSlideBraceContra :: Int32
kScaleScalar = 0
kSlideNode = 1
kScaleSubTreeTime = 2
kPulley = 3
kScaleBranchRate = 4
kScaleSubTreeRate = 5
kScaleNormTree = 6
kScaleVarTree = 7
kScaleVarTreeAuto = 8
kScaleContrarily = 9
kSlideNodeContra = 10
kScaleSubTreeContra = 11
kSlideRootContra = 12
kScaleRatesTreeContra = 13
kSlideBrace = 14
kSlideBraceContra = 15

-- | Per node in pre-order: (id, depth of the path from the root, number of nodes / of inner nodes of its sub tree, levels of its sub
-- tree ('T.depth': a leaf has 1), number of children).
data NodeInfo = NodeInfo {niId :: Int, niPath :: Int, niSize :: Int, niInner :: Int, niLevels :: Int, niKids :: Int}

nodeInfos :: T.Tree e a -> [NodeInfo]
nodeInfos t0 = go 0 0 t0 []
  where
    go i d t acc =
      let me = NodeInfo i d (length t) (nInner t) (T.depth t) (length (T.forest t))
          step (j, f) c = (j + length c, f . go j (d + 1) c)
          (_, rest) = foldl' step (i + 1, id) (T.forest t)
       in me : rest acc
    nInner t = if null (T.forest t) then 0 else 1 + sum (map nInner (T.forest t))

-- | weightNBranches, app/Definitions.hs:127-130.
weightNBranches :: Int -> Int
weightNBranches n = floor (logBase 1.3 (fromIntegral n :: Double))

-- | @proposals bs calibrationsAvailable x Nothing@ (app/Definitions.hs:256-278) as table rows, in the reference's order.
-- braceSizes: per brace of @bs@ (in order) the number of braced nodes and the number of their daughters (PDimension of the two
-- brace proposals, lib/Mcmc/Tree/Proposal/Brace.hs:37-61, 98-156); the brace INDEX is the one of the prior handle.
proposalTable :: [(Int, Int)] -> Bool -> T.Tree e a -> [ProposalRow]
proposalTable braceSizes calibrationsAvailable t =
  [ row "Time birth rate" kScaleScalar 0 0 0 0 1 10 0 w,
    row "Time death rate" kScaleScalar 1 0 0 0 1 10 0 w,
    row "Rate mean" kScaleScalar 3 0 0 0 1 10 0 w,
    row "Rate variance" kScaleScalar 4 0 0 0 1 10 0 w,
    row "Rates and time tree" kScaleRatesTreeContra 0 (nInnerAll - 1) 0 1 (nInnerAll - 1 + 2) 0.1 0 w
  ]
    ++ proposalsTimeTree
    ++ proposalsRateTree
    ++ proposalsContra
    ++ (if calibrationsAvailable then proposalsChangingTimeHeight else [])
  where
    row nm k v a b j d p0 p1 wt = ProposalRow nm k (fromIntegral v) (fromIntegral a) (fromIntegral b) j (fromIntegral d) p0 p1 wt
    infos = nodeInfos t
    n = length infos
    w = weightNBranches n
    nInnerAll = niInner (head infos)
    inner = filter ((> 0) . niKids) infos
    childrenOfRoot = (== 1) . niPath -- :133-134
    otherNodes = (> 1) . niPath -- :137-138
    subW i = min (3 + niLevels i - 2) 8 -- pWeight 3 .. pWeight 8 by the depth of the sub tree
    [l, r] = case filter childrenOfRoot infos of
      xs@[_, _] -> xs
      _ -> error "proposalTable: Tree is not bifurcating."
    -- proposalsTimeTree, :145-166
    timePs hn tag j =
      [row (tag <> " Time tree") kSlideNode (niId i) 0 0 j 1 0.01 0 5 | i <- inner, hn i]
        ++ [row (tag <> " Time tree") kScaleSubTreeTime (niId i) (niInner i) 0 j (niInner i) 0.01 0 (subW i) | i <- inner, hn i]
    proposalsTimeTree =
      [row "[R] Time tree" kPulley 0 (niInner l) (niInner r) 1 (niInner l + niInner r) 0.01 0 6 | niKids l > 0, niKids r > 0]
        ++ timePs childrenOfRoot "[R]" 1
        ++ timePs otherNodes "[O]" 0
        ++ [row "[B] Time tree" kSlideBrace bi 0 0 0 nb 0.01 0 5 | (bi, (nb, _)) <- zip [0 :: Int ..] braceSizes]
    -- proposalsRateTree, :180-201
    ratePs hn tag j =
      [row (tag <> " Rate tree") kScaleBranchRate (niId i) 0 0 j 1 100 0 3 | i <- infos, hn i]
        ++ [row (tag <> " Rate tree") kScaleSubTreeRate (niId i) (niSize i) 0 j (niSize i) 100 0 (subW i) | i <- inner, hn i]
    proposalsRateTree =
      [ row "[R] Rate mean, Rate tree" kScaleNormTree 3 0 0 1 n 100 0 w,
        row "[R] Rate variance, Rate tree" kScaleVarTree 0 0 0 1 n 100 0 w,
        row "[R] Rate variance, Rate tree" kScaleVarTreeAuto 0 0 0 1 n 100 0 w
      ]
        ++ ratePs childrenOfRoot "[R]" 1
        ++ ratePs otherNodes "[O]" 0
    -- proposalsTimeRateTreeContra, :204-221
    contraPs hn tag j =
      [row (tag <> " Trees") kSlideNodeContra (niId i) 0 0 j (1 + 1 + niKids i) 0.1 0 (subW i) | i <- inner, hn i]
        ++ [row (tag <> " Trees") kScaleSubTreeContra (niId i) (niInner i) (niSize i) j (niInner i + niSize i) 0.1 0 (subW i) | i <- inner, hn i]
    proposalsContra =
      contraPs childrenOfRoot "[C] [R]" 1
        ++ contraPs otherNodes "[C] [O]" 0
        ++ [row "[C] [B] Trees" kSlideBraceContra bi 0 0 0 (2 * nb + nd) 0.1 0 5 | (bi, (nb, nd)) <- zip [0 :: Int ..] braceSizes]
    -- proposalsChangingTimeHeight, :241-253
    proposalsChangingTimeHeight =
      [ row "Time height" kScaleScalar 2 0 0 0 1 3000 0 w,
        row "Time height, rate mean" kScaleContrarily 0 0 0 0 2 10 0.1 w,
        row "[R] Time height, Rate tree" kScaleNormTree 2 0 0 1 n 100 0 w,
        row "[R] Trees" kSlideRootContra 0 nInnerAll 0 1 (1 + nInnerAll + 2) 10 0 w
      ]

-- | mcmc's default order of a cycle (@RandomO@): every iteration executes each proposal @weight@ times in a freshly shuffled
-- order.  @nIter@ iterations, flattened: what @mcd_mh_run@ takes as schedule.
cycleSchedule :: StatefulGen g m => [ProposalRow] -> Int -> g -> m (VS.Vector Int32)
cycleSchedule ps nIter g = VS.concat <$> replicateM nIter one
  where
    base = concat [replicate (prWeight p) i | (i, p) <- zip [0 :: Int32 ..] ps]
    one = shuffle base
    shuffle xs = go (length xs) xs []
      where
        go 0 _ acc = pure (VS.fromList acc)
        go k ys acc = do
          j <- uniformRM (0, k - 1) g
          let (a, b : c) = splitAt j ys
          go (k - 1) (a ++ c) (b : acc)

-- ---------------------------------------------------------------------------------------------------------------------------------
-- The sampler
-- ---------------------------------------------------------------------------------------------------------------------------------
-- | What 'getLikelihoodHandle' made of the @.data@ record: the dense factor or the sparse precision matrix on the device.
data LikelihoodHandle = DenseTree (Ptr McdTree) | SparseTree (Ptr McdSparseTree)

data GpuSampler = GpuSampler
  { gsHandle :: Ptr McdMh,
    gsTable :: [ProposalRow],
    gsChains :: Int,
    gsNodes :: Int,
    gsTemplate :: I -- the topology and labels every fetched state is poured into
  }

-- | Create the driver for @chains@ chains that all start at @x0@ ('initWith', app/Definitions.hs:96-123), run the action, free it.
withGpuSampler :: LikelihoodHandle -> Ptr McdPrior -> [ProposalRow] -> Int -> Word64 -> I -> (GpuSampler -> IO a) -> IO a
withGpuSampler lik prior table chains seed x0 act =
  alloca $ \pp ->
    withArrays table $ \np kind node n1 n2 jr dm p0 p1 -> do
      check "mcd_mh_create" =<< case lik of
        DenseTree t -> c_mh_create pp t prior np kind node n1 n2 jr dm p0 p1 (fromIntegral chains) seed
        SparseTree t -> c_mh_create_sparse pp t prior np kind node n1 n2 jr dm p0 p1 (fromIntegral chains) seed
      h <- peek pp
      let nn = length (T.branches (getHeightTree (x0 ^. timeTree)))
          s = GpuSampler h table chains nn x0
      setStates s (replicate chains x0)
      r <- act s
      c_mh_destroy h
      pure r
  where
    withArrays ps k =
      VS.unsafeWith (VS.fromList (map prKind ps)) $ \a ->
        VS.unsafeWith (VS.fromList (map prNode ps)) $ \b ->
          VS.unsafeWith (VS.fromList (map prN1 ps)) $ \c ->
            VS.unsafeWith (VS.fromList (map prN2 ps)) $ \d ->
              VS.unsafeWith (VS.fromList (map prJacRoot ps)) $ \e ->
                VS.unsafeWith (VS.fromList (map prDim ps)) $ \f ->
                  VS.unsafeWith (VS.fromList (map (realToFrac . prP0) ps)) $ \g ->
                    VS.unsafeWith (VS.fromList (map (realToFrac . prP1) ps)) $ \h ->
                      k (fromIntegral (length ps)) a b c d e f g h

-- the seven fields of 'I' as chain-major arrays (heights / rates: the pre-order 'branches' of the two trees, app/State.hs:70-100)
setStates :: GpuSampler -> [I] -> IO ()
setStates s xs =
  let col f = VS.fromList (map (realToFrac . f) xs) :: VS.Vector CDouble
      rows f = VS.fromList (concatMap (map realToFrac . f) xs) :: VS.Vector CDouble
      hs x = T.branches (getHeightTree (x ^. timeTree))
      rs x = T.branches (getLengthTree (x ^. rateTree))
   in VS.unsafeWith (col (^. timeBirthRate)) $ \pb ->
        VS.unsafeWith (col (^. timeDeathRate)) $ \pd ->
          VS.unsafeWith (col (^. timeHeight)) $ \pt ->
            VS.unsafeWith (rows hs) $ \ph ->
              VS.unsafeWith (col (^. rateMean)) $ \pm ->
                VS.unsafeWith (col (^. rateVariance)) $ \pv ->
                  VS.unsafeWith (rows rs) $ \pr ->
                    check "mcd_mh_set_state" =<< c_mh_set_state (gsHandle s) pb pd pt ph pm pv pr (fromIntegral (gsNodes s))

-- the chains' current states as values of 'I': the template's trees relabelled in pre-order
getStates :: GpuSampler -> IO [I]
getStates s = do
  let b = gsChains s
      nn = gsNodes s
  sc <- VSM.new (5 * b)
  hh <- VSM.new (b * nn)
  rr <- VSM.new (b * nn)
  VSM.unsafeWith sc $ \p ->
    VSM.unsafeWith hh $ \ph ->
      VSM.unsafeWith rr $ \pr ->
        check "mcd_mh_get_state"
          =<< c_mh_get_state (gsHandle s) p (p `advancePtr` b) (p `advancePtr` (2 * b)) ph (p `advancePtr` (3 * b)) (p `advancePtr` (4 * b)) pr (fromIntegral nn)
  scv <- VS.freeze sc
  hv <- VS.freeze hh
  rv <- VS.freeze rr
  pure [pourState s (\k -> realToFrac (scv VS.! (k * b + i))) (VS.slice (i * nn) nn hv) (VS.slice (i * nn) nn rv) | i <- [0 .. b - 1]]

-- one state as a value of 'I': the five scalars (birth, death, tH, rMu, rVar) by index, heights and rates in pre-order
pourState :: GpuSampler -> (Int -> Double) -> VS.Vector CDouble -> VS.Vector CDouble -> I
pourState s at hs rs =
  x0
    & timeBirthRate .~ at 0
    & timeDeathRate .~ at 1
    & timeHeight .~ at 2
    & rateMean .~ at 3
    & rateVariance .~ at 4
    & timeTree .~ HeightTree (relabel (getHeightTree (x0 ^. timeTree)) (list hs))
    & rateTree .~ LengthTree (relabel (getLengthTree (x0 ^. rateTree)) (list rs))
  where
    x0 = gsTemplate s
    list v = map realToFrac (VS.toList v) :: [Double]
    -- new branch labels in pre-order (the order of 'T.branches')
    relabel t ls = case T.setBranches ls t of
      Just t' -> t'
      Nothing -> error "pourState: wrong number of branch labels."

-- | @--hamiltonian@ ('maybeHamiltonianProposal', app/Definitions.hs:272-278; 'nutsWith', app/Hamiltonian.hs:95-105): for the duration
-- of the action every iteration of every loop of this module ('runMetropolisHastingsGreenGpu', 'runRecorded', ...) begins with one NUTS
-- transition of every chain on the leapfrog handle @hmc@ (made by "McmcDate.Gpu" over the same likelihood and prior, as many chains),
-- and the shuffled cycle follows.  The reference shuffles the proposal into the cycle; here it is the first position, so the monitors
-- and the recorder see complete iterations.
--   eps       step sizes, one per chain (tuned beforehand: @mcd_hmc_take_state@ + @mcd_hmc_nuts_warmup@ / @_warmup_dense@ on @hmc@)
--   invMass   @Just@ the diagonal inverse masses (length @mcd_hmc_dim@), or @Nothing@: the dense metric set on @hmc@
--   seed      the sampler's seed xor a constant of the host's, so that the NUTS streams stay apart from the proposals' streams
-- Returns the action's result and the mean acceptance statistic, mean tree depth and number of divergent transitions per chain.
-- The transitions are launched as @hmc@'s form says: 'setHamiltonianTransitionForm' beforehand.
withHamiltonian :: GpuSampler -> Ptr McdHmc -> [Double] -> Maybe [Double] -> Int -> Word64 -> IO a -> IO (a, [(Double, Double, Int)])
withHamiltonian s hmc eps invMass maxDepth seed act =
  VS.unsafeWith (VS.fromList (map realToFrac eps)) $ \pe ->
    withMass $ \pm -> do
      check "mcd_mh_attach_hamiltonian" =<< c_mh_attach_hamiltonian (gsHandle s) hmc pe pm (fromIntegral maxDepth) seed 0
      r <- act
      let b = gsChains s
      al <- VSM.new b
      dp <- VSM.new b
      dv <- VSM.new b
      n <- alloca $ \pn -> do
        VSM.unsafeWith al $ \pa -> VSM.unsafeWith dp $ \pd -> VSM.unsafeWith dv $ \pv ->
          check "mcd_mh_hamiltonian_stats" =<< c_mh_hamiltonian_stats (gsHandle s) pn pa pd nullPtr pv 0
        peek pn
      check "mcd_mh_detach_hamiltonian" =<< c_mh_detach_hamiltonian (gsHandle s)
      av <- VS.freeze al
      dpv <- VS.freeze dp
      dvv <- VS.freeze dv
      let k = fromIntegral (max 1 n) :: Double
      pure (r, [(realToFrac (av VS.! i) / k, fromIntegral (dpv VS.! i) / k, fromIntegral (dvv VS.! i)) | i <- [0 .. b - 1]])
  where
    withMass k = case invMass of
      Nothing -> k nullPtr
      Just ms -> VS.unsafeWith (VS.fromList (map realToFrac ms)) k

-- | How the leapfrog handle launches a NUTS transition, for 'withHamiltonian' and every other caller: @False@ the rounds of three
-- launches (the default), @True@ one launch per transition (@mcd_hmc_set_transition_form@; the datasets of the reference, 9 .. 47
-- distances, are all eligible).  The library refuses a handle it cannot serve that way (a sparse likelihood, more than 64 distances,
-- the across-chains form of a dense metric) and leaves it as it was; the chains' bits do not depend on the choice.
setHamiltonianTransitionForm :: Ptr McdHmc -> Bool -> IO ()
setHamiltonianTransitionForm hmc oneLaunch =
  check "mcd_hmc_set_transition_form" =<< c_hmc_set_transition_form hmc (if oneLaunch then 1 else 0)

-- one block of iterations through the shuffled cycle; accumulate: add the node ages to the running sums after every iteration
runBlock :: StatefulGen g IO => GpuSampler -> g -> Int -> Bool -> IO ()
runBlock s g nIter accumulate = do
  sched <- cycleSchedule (gsTable s) nIter g
  let steps = sum (map prWeight (gsTable s))
  VS.unsafeWith sched $ \p ->
    check "mcd_mh_run" =<< c_mh_run (gsHandle s) p (fromIntegral nIter) (fromIntegral steps) (if accumulate then 1 else 0) nullPtr nullPtr

-- | Replacement of @runMetropolisHastingsGreen@'s @MhgA@ branch (app/Main.hs:460-475) for B chains in lock step.
--   burnInPeriods   the tuning periods of 'Definitions.burnIn' (fast ++ slow: [10, 10, 10, 20 .. 130] ++ [100, 120 .. 400], :420-424)
--   iterations      'Definitions.iterations' (8000, :440-441)
--   period          the monitors' period (2, :288-417)
--   onSample        the monitor action: iteration number and the chains' states (the reference's 'monitor' executes on an 'I'; a host
--                   that wants one output directory per chain maps over the list)
runMetropolisHastingsGreenGpu :: StatefulGen g IO => GpuSampler -> g -> [Int] -> Int -> Int -> (Int -> [I] -> IO ()) -> IO ()
runMetropolisHastingsGreenGpu s g burnInPeriods iterations period onSample = do
  getStates s >>= onSample 0
  it <- newCounter
  forM_ burnInPeriods $ \p -> do
    blocks it p False
    check "mcd_mh_tune" =<< c_mh_tune (gsHandle s) -- mcmc's auto tuning at the end of a tuning period
  check "mcd_mh_reset_age_sums" =<< c_mh_reset_age_sums (gsHandle s)
  blocks it iterations True
  where
    newCounter = VSM.replicate 1 (0 :: Int)
    blocks it n acc = go n
      where
        go left = when (left > 0) $ do
          let k = min period left
          runBlock s g k acc
          VSM.modify it (+ k) 0
          i <- VSM.read it 0
          when (k == period) (getStates s >>= onSample i)
          go (left - k)

-- | What a load takes from a blob: everything (@continue@, app/Main.hs:494-509) or states, posterior terms and tuning parameters only
-- (@--init-from-save@, @mhgLoadUnsafe@, :424-440; MCD_CKPT_FULL / MCD_CKPT_STATE_TUNING of the header).
data CheckpointMode = CheckpointFull | CheckpointStateAndTuning

-- | The sampler between two runs as one blob (mcd_mh_save): state, posterior terms, temperatures, tuning parameters and counters, age sums,
-- the step counter of the random streams, the recorder's counts.  The host writes it beside its own generator @g@ and iteration count, as
-- @mcmc@ does with @Settings ... Save@.  The chains do not change.
saveSampler :: GpuSampler -> IO (VS.Vector Word8)
saveSampler s = do
  n <- alloca $ \pn -> (check "mcd_mh_save_size" =<< c_mh_save_size (gsHandle s) pn) >> peek pn
  buf <- VSM.new (fromIntegral n)
  VSM.unsafeWith buf $ \p -> alloca $ \pw -> check "mcd_mh_save" =<< c_mh_save (gsHandle s) p n pw
  VS.unsafeFreeze buf

-- | The blob of 'saveSampler' into a sampler made by the same 'withGpuSampler' call (tree, likelihood, prior, table, chains, seed): no
-- 'setStates' is needed.  A refused blob (the error names the mismatch) leaves the sampler untouched.
loadSampler :: GpuSampler -> CheckpointMode -> VS.Vector Word8 -> IO ()
loadSampler s mode blob =
  VS.unsafeWith blob $ \p ->
    check "mcd_mh_load" =<< c_mh_load (gsHandle s) p (fromIntegral (VS.length blob)) (case mode of CheckpointFull -> 0; CheckpointStateAndTuning -> 1)

-- | Counterpart of @continueMetropolisHastingsGreen@ (app/Main.hs:494-509): the sampling phase of 'runMetropolisHastingsGreenGpu' goes on
-- from a blob saved behind @done@ of its iterations, for the @iterations - done@ that are left, on the generator @g@ the host saved beside
-- it.  The samples are those of the uninterrupted run, bit for bit.
continueMetropolisHastingsGreenGpu :: StatefulGen g IO => GpuSampler -> g -> VS.Vector Word8 -> Int -> Int -> Int -> (Int -> [I] -> IO ()) -> IO ()
continueMetropolisHastingsGreenGpu s g blob done iterations period onSample = do
  loadSampler s CheckpointFull blob
  go done
  where
    go i = when (i < iterations) $ do
      let k = min period (iterations - i)
      runBlock s g k True
      when (k == period) (getStates s >>= onSample (i + k))
      go (i + k)

-- | Replacement of @runMarginalLikelihood@ (app/Main.hs:511-543: @marginalLikelihood mlS p l c m i g@) over a sampler of nPoints x
-- replicates chains: chain b runs at the path point b mod nPoints with the target prior x likelihood^beta (mcd_mh_set_power), all points in
-- lock step -- no walk along the path.
--   nPoints         'Definitions.nPoints' (128, :452-453); the sampler's chain count must be a multiple
--   burnInPeriods   'Definitions.repetitiveBurnIn' (fast ++ slow: [20, 40, 60, 80] ++ replicate 6 100, :461-465): every chain tunes at its own beta
--   iterations      'Definitions.iterationsMarginalLh' (4000, :448-449); every @period@-th is recorded on the device
-- Returns (ln Z by stepping stones, its standard error, ln Z by thermodynamic integration, its standard error): out[4] of
-- mcd_mh_record_marginal, the errors over the replicates (NaN with one replicate).  The points (k / (K - 1))^(1 / 0.3), the estimators and
-- the errors are the library's definitions (include/mcmcdate_mvn.h), unpinned against package mcmc's own marginalLikelihood.
runMarginalLikelihoodGpu :: StatefulGen g IO => GpuSampler -> g -> Int -> [Int] -> Int -> Int -> IO (Double, Double, Double, Double)
runMarginalLikelihoodGpu s g nPoints burnInPeriods iterations period = do
  let b = gsChains s
      k1 = fromIntegral (nPoints - 1) :: Double
      betas = VS.generate nPoints $ \k ->
        if k == 0 then 0 else if k == nPoints - 1 then 1 else CDouble ((fromIntegral k / k1) ** (1 / 0.3))
      perChain = VS.generate b (\c -> betas VS.! (c `mod` nPoints))
  when (b `mod` nPoints /= 0) $ error "runMarginalLikelihoodGpu: the chains are not whole groups of nPoints."
  VS.unsafeWith perChain $ \p -> check "mcd_mh_set_power" =<< c_mh_set_power (gsHandle s) p
  forM_ burnInPeriods $ \n -> do
    runBlock s g n False
    check "mcd_mh_tune" =<< c_mh_tune (gsHandle s)
  check "mcd_mh_record_begin" =<< c_mh_record_begin (gsHandle s) (fromIntegral period) (fromIntegral (iterations `div` period))
  runBlock s g iterations False
  out <- VSM.new 4
  VS.unsafeWith betas $ \pb -> VSM.unsafeWith out $ \po -> alloca $ \pn ->
    check "mcd_mh_record_marginal" =<< c_mh_record_marginal (gsHandle s) (fromIntegral nPoints) pb 0 (-1) pn nullPtr nullPtr po
  check "mcd_mh_record_end" =<< c_mh_record_end (gsHandle s)
  [a, ea, t, et] <- mapM (fmap realToFrac . VSM.read out) [0 .. 3]
  pure (a, ea, t, et)

-- | 'runMetropolisHastingsGreenGpu' with the samples kept on the device (the recorder of include/mcmcdate_mvn.h): every tuning period
-- and the iterations run in calls of up to @chunk@ iterations instead of @period@, and the monitor action is called from what
-- @mcd_mh_record_fetch@ returns after each call -- the same iteration numbers as long as every tuning period is a multiple of
-- @period@ (the reference's are all even, its period is 2: the old loop restarts its blocks at every tuning period and skips a short
-- last block, the recorder samples on global multiples of @period@) and, the rounding of the incremental likelihood apart
-- (every call restarts it from a full product), the same states.  The recorder counts iterations from its begin, which is the start
-- of the run here, so the iteration numbers are the loop's own.
runRecorded :: StatefulGen g IO => GpuSampler -> g -> [Int] -> Int -> Int -> Int -> (Int -> [I] -> IO ()) -> IO ()
runRecorded s g burnInPeriods iterations period chunk onSample = do
  getStates s >>= onSample 0
  let cap = (chunk + period - 1) `div` period -- what one call can add at most
  check "mcd_mh_record_begin" =<< c_mh_record_begin (gsHandle s) (fromIntegral period) (fromIntegral cap)
  forM_ burnInPeriods $ \p -> do
    chunks cap p False
    check "mcd_mh_tune" =<< c_mh_tune (gsHandle s)
  check "mcd_mh_reset_age_sums" =<< c_mh_reset_age_sums (gsHandle s)
  chunks cap iterations True
  check "mcd_mh_record_end" =<< c_mh_record_end (gsHandle s)
  where
    b = gsChains s
    nn = gsNodes s
    chunks cap n acc = go n
      where
        go left = when (left > 0) $ do
          let k = min chunk left
          runBlock s g k acc
          drain cap
          go (left - k)
    drain cap = do
      its <- VSM.new cap
      sc <- VSM.new (cap * b * 5)
      hh <- VSM.new (cap * b * nn)
      rr <- VSM.new (cap * b * nn)
      n <- alloca $ \pn -> do
        VSM.unsafeWith its $ \pi' -> VSM.unsafeWith sc $ \ps -> VSM.unsafeWith hh $ \ph -> VSM.unsafeWith rr $ \pr ->
          check "mcd_mh_record_fetch" =<< c_mh_record_fetch (gsHandle s) (fromIntegral cap) pn pi' ps ph pr nullPtr nullPtr
        fromIntegral <$> peek pn
      iv <- VS.freeze its
      scv <- VS.freeze sc
      hv <- VS.freeze hh
      rv <- VS.freeze rr
      forM_ [0 .. n - 1] $ \k ->
        onSample
          (fromIntegral (iv VS.! k))
          [ pourState s (\f -> realToFrac (scv VS.! ((k * b + i) * 5 + f))) (VS.slice ((k * b + i) * nn) nn hv) (VS.slice ((k * b + i) * nn) nn rv)
            | i <- [0 .. b - 1]
          ]

-- | Posterior summaries and convergence diagnostics of the samples waiting in the recorder, computed on the device where they lie
-- (@mcd_mh_record_summary@; call it between @mcd_mh_record_begin@ and @_end@, e.g. from a variant of 'runRecorded' that fetches
-- nothing): the samples @[skip, skip + n)@ (all after @skip@ when @n < 0@), the lag cap @maxLag@ of the effective sample size (odd, at
-- most 255 and half the window less one; 0: none).  Returns the number of samples used and, per quantity -- ages @tH * h_v@ per node,
-- rates per node, birth, death, tH, rMu, rVar, ln prior, ln likelihood, ln jacobianRootBranch, ln posterior -- the nine columns mean,
-- maximum-likelihood variance, minimum, maximum, the two order statistics of the 95 % interval of
-- @scripts/trees-monitor-summary-ultrametric@, split R-hat, effective sample size, last lag of Geyer's sum.
recordSummary :: GpuSampler -> Int -> Int -> Int -> IO (Int, [[Double]])
recordSummary s skip n maxLag = do
  q <- alloca $ \pq -> do
    check "mcd_mh_record_quantities" =<< c_mh_record_quantities (gsHandle s) pq
    fromIntegral <$> peek pq
  out <- VSM.new (q * 9)
  used <- alloca $ \pn -> do
    VSM.unsafeWith out $ \po ->
      check "mcd_mh_record_summary"
        =<< c_mh_record_summary (gsHandle s) (fromIntegral skip) (fromIntegral n) (fromIntegral maxLag) pn po nullPtr
    fromIntegral <$> peek pn
  v <- VS.freeze out
  pure (used, [[realToFrac (v VS.! (i * 9 + j)) | j <- [0 .. 8]] | i <- [0 .. q - 1]])

-- | @mc3 (MC3Settings (NChains nChains) (SwapPeriod swapPeriod) (NSwaps nSwaps))@ (app/Main.hs:476-478) over the same driver: the
-- global set of chains is cut into groups of @nChains@ consecutive chains with the ladder of reciprocal temperatures @betas@ (head = 1);
-- the swap phase runs on the device.  The monitor action receives the COLD chain of every group.
runMc3Gpu :: StatefulGen g IO => GpuSampler -> g -> Int -> Int -> Int -> [Double] -> Word64 -> [Int] -> Int -> (Int -> [I] -> IO ()) -> IO ()
runMc3Gpu s g nChains swapPeriod nSwaps betas seed burnInPeriods iterations onSample = do
  VS.unsafeWith (VS.fromList (map realToFrac betas)) $ \pb ->
    check "mcd_mh_mc3_init" =<< c_mh_mc3_init (gsHandle s) (fromIntegral nChains) pb (fromIntegral (gsChains s)) seed
  it <- VSM.replicate 1 (0 :: Int)
  let periods n acc = go n
        where
          go left = when (left > 0) $ do
            let k = min swapPeriod left
            runBlock s g k acc
            when (k == swapPeriod) $ do
              -- one GPU holds every chain: gathered = nullPtr (sharded: the buffer mcd_shard_allgather made, see McmcDate.Gpu)
              check "mcd_mh_mc3_swap" =<< c_mh_mc3_swap (gsHandle s) (fromIntegral nSwaps) nullPtr 1 (fromIntegral (gsChains s))
              VSM.modify it (+ k) 0
              i <- VSM.read it 0
              cold >>= onSample i
            go (left - k)
  forM_ burnInPeriods $ \p -> periods p False >> (check "mcd_mh_tune" =<< c_mh_tune (gsHandle s))
  periods iterations True
  where
    cold = do
      xs <- getStates s
      rk <- VSM.new (gsChains s)
      VSM.unsafeWith rk $ \p -> check "mcd_mh_mc3_get" =<< c_mh_mc3_get (gsHandle s) p nullPtr nullPtr nullPtr
      rv <- VS.freeze rk
      pure [x | (x, r) <- zip xs (VS.toList rv), r == (0 :: Int32)]

-- | Mean and variance of every node's absolute age over the accumulated iterations, per chain: what
-- @scripts/trees-monitor-summary-ultrametric@ computes from the time-tree monitor file (:149-175), without writing 8000 trees.
nodeAgeSummary :: GpuSampler -> IO [[(Double, Double)]]
nodeAgeSummary s = do
  let b = gsChains s
      nn = gsNodes s
  sm <- VSM.new (b * nn)
  sq <- VSM.new (b * nn)
  cnt <- alloca $ \pn -> do
    VSM.unsafeWith sm $ \p1 -> VSM.unsafeWith sq $ \p2 -> check "mcd_mh_get_age_sums" =<< c_mh_get_age_sums (gsHandle s) p1 p2 pn
    peek pn
  a <- VS.freeze sm
  q <- VS.freeze sq
  let k = fromIntegral cnt :: Double
      stat i = let m = realToFrac (a VS.! i) / k in (m, realToFrac (q VS.! i) / k - m * m)
  pure [[stat (c * nn + v) | v <- [0 .. nn - 1]] | c <- [0 .. b - 1]]

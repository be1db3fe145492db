"""The sweep behind ATX_PARCEL_NEWTON_STEPS (include/atx_parcel.h): the Newton steps of the moist adiabat in 80-bit extended arithmetic,
so that the step and not its rounding is measured, over starts at 1080 .. 300 hPa, 230 .. 320 K, seven humidities, 400 levels each up to
50 hPa.  Prints, per start pressure, the last step that still moves T by one float64 ulp or more, and how often a step met its cap.

    python tools/parcel_newton_sweep.py
"""
import numpy as np
L=np.longdouble
RD,RV=L(287.0597),L(461.5250); eps=RD/RV; LN1E5=L(11.512925464970229); KAPPA=L(2)/L(7)
def lnthe(lnT,TL,r,lnp): return (lnT+(L(0.2854)*(1-L(0.28)*r))*(LN1E5-lnp))+((L(3.376)/TL-L(0.00254))*(1000*r))*(1+L(0.81)*r)
def es(T): return L(611.21)*np.exp(L(17.502)*(T-L(273.16))/(T-L(32.19)))
worst=0; capped=0
for ps in (108000.,100000.,85000.,70000.,50000.,30000.):
  Ts=np.linspace(230,320,181).astype(L)[:,None,None]
  rh=np.array([1.0,0.999,0.9,0.5,0.1,1e-3,1e-6]).astype(L)[None,:,None]
  pk=np.geomspace(5000.,ps,400).astype(L)[None,None,:]
  e=rh*es(Ts); e=np.minimum(e,L(0.9)*L(ps)/ (1+0*e))
  r=eps*e/(L(ps)-e)
  e2=L(ps)*r/(eps+r); lnT=np.log(Ts)
  TL=L(2840)/((L(3.5)*lnT-np.log(e2/100))-L(4.805))+55
  target=lnthe(lnT,TL,r,np.log(L(ps)))
  pL=L(ps)*np.exp(L(3.5)*np.log(TL/Ts))
  T=Ts*np.exp(KAPPA*np.log(pk/L(ps)))+0*r
  moist=(pk<pL)&(e<0.5*ps)
  lnp=np.log(pk); lnh=np.log(pk/L(1222.42)); cap=(L(32.19)*lnh-L(4780.84632))/(lnh-L(17.502))
  need=np.zeros(T.shape,int)
  for it in range(1,40):
    e_s=es(T); pe=pk-e_s; rr=eps*e_s/pe
    F=lnthe(np.log(T),T,rr,lnp)-target
    d=T-L(32.19); dr=rr*(pk/pe)*(L(4217.45694)/(d*d)); w=1000*rr*(1+L(0.81)*rr)
    dF=((1/T-(L(0.079912)*dr)*(LN1E5-lnp))-(L(3.376)/(T*T))*w)+((L(3.376)/T-L(0.00254))*(1000*dr))*(1+L(1.62)*rr)
    Tn=T-F/dF
    capped+=int(((Tn>=cap)&moist).sum())
    Tn=np.minimum(Tn,cap)
    moved=np.abs(Tn-T)>=np.spacing(np.abs(T).astype(np.float64)).astype(L)
    need=np.where(moved&moist,it,need)   # step `it` still moved T by >= 1 ulp
    T=Tn
  print(ps, "steps needed max", need.max(), "bad", int((~np.isfinite(T)&moist).sum()), "hist", np.bincount(need[moist].ravel()))
  worst=max(worst,need.max())
print("N =",worst, "capped",capped)
